"""Array-backed batch API of the scheme (SURVEY.md 8f rows N1 + N2): keys, challenges and signatures
are int32 arrays instead of lists of polynomial objects, hashing/decoding runs in the C host pipeline
(hostpipe) and all algebra on the device.  Results are the same integers the object API
(fusion.fusion.keygen / sign / aggregate / verify) produces -- tests/test_gpu_batch_scheme.py checks both
against the reference's golden arrays.

Layouts: sk_hat [N][2][l][d] (left rows then right rows), vk [N][2][d], c_hat / alpha_hat [N][d],
sig [N][l][d], aggregate [l][d]; all int32, centred.
"""
import numpy as np

from . import hostpipe
from ._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED, FusionHipError
from .context import (Context, DeviceArray, DeviceScope, ENCODING_REASONS, SIGNATURE_REASONS, VERDICT_REASONS,  # noqa: F401 (re-exported)
                      get_context)

# The bound of ONE honest signature, ||INTT(sigma)||_inf <= beta_sk * (1 + min(degree, omega_ch) * CH_BD): the reference's
# VF_BD_INTERMEDIATE_128 / _256 (fusion.py:59-64; fusion/fusion.py keeps them under the same names), which it only uses to
# build beta_vf.  A table and not a formula over the params: CH_BD_128 = 3 is not the live beta_ch (1).
_SIGNATURE_BOUNDS = {128: 4264, 256: 3172}


def signature_bound(params):
    """the infinity-norm bound of a single signature for params.secpar (4264 at 128, 3172 at 256); no device needed.  Any
    other parameter set has no such constant: FusionHipError(FZ_E_BADARG), pass `beta` explicitly instead."""
    secpar = getattr(params, "secpar", None)
    if secpar not in _SIGNATURE_BOUNDS:
        raise FusionHipError(FZ_E_BADARG, f"no single-signature bound for secpar {secpar!r}: pass beta explicitly")
    return _SIGNATURE_BOUNDS[secpar]


# the kinds of the compact byte encoding: params -> (rows of a record, coefficient domain?, bound B)
_ENCODING_KINDS = {
    "vk": lambda p: (2, False, (p.modulus - 1) // 2),
    "signature": lambda p: (p.num_rows_sk, True, signature_bound(p)),
    "aggregate": lambda p: (p.num_rows_sk, True, int(p.beta_vf)),
    # a signing key's [2][l][d] rows, left half first: |s| <= beta_sk for every key keygen can make (omega_sk = d: no weight bound)
    "secret": lambda p: (2 * p.num_rows_sk, True, int(p.beta_sk)),
}


def _encoding(params, kind):
    """-> (rows, coef, bound, w, record_bytes) of `kind` for params; FusionHipError(FZ_E_BADARG) for an unknown kind or secpar"""
    if kind not in _ENCODING_KINDS:
        raise FusionHipError(FZ_E_BADARG, f"unknown encoding kind {kind!r}: one of {sorted(_ENCODING_KINDS)}")
    signature_bound(params)                                    # the secpar check: only the reference's two parameter sets
    rows, coef, bound = _ENCODING_KINDS[kind](params)
    w = (2 * bound).bit_length()
    return rows, coef, bound, w, rows * params.degree * w // 8


def encoded_size(params, kind):
    """bytes of one record of `kind` ("vk", "signature", "aggregate" or "secret") in the compact byte encoding; no device
    needed"""
    return _encoding(params, kind)[4]


def _records_input(kind, data, rb):
    """the byte input of decode / aggregate_encoded (bytes, bytearray, memoryview, a uint8 numpy array or a uint8 DeviceArray)
    -> (a uint8 numpy array or the DeviceArray, N); FusionHipError(FZ_E_BADARG) unless it is N whole records of rb bytes"""
    if isinstance(data, DeviceArray):
        if data.dtype != np.uint8:
            raise FusionHipError(FZ_E_BADARG, f"device array of {data.dtype}: uint8 expected")
        nbytes = int(np.prod(data.shape))
    else:
        data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(data)
        if data.dtype != np.uint8:
            raise FusionHipError(FZ_E_BADARG, f"array of {data.dtype}: uint8 expected")
        nbytes = data.size
    if nbytes % rb:
        raise FusionHipError(FZ_E_BADARG, f"{nbytes} bytes are not a whole number of {rb}-byte {kind!r} records")
    return data, nbytes // rb


def screened_alpha_coefficients(P, L, R, pre, c_hat, valid=None, threads=None, order=None):
    """hash_ag without the transforms (fusion.py:632-652) for ONE aggregate of the signers with valid[i] set: sort them by
    str(vk) (fusion.py:661-663, :693), the one serial SHAKE-256 over the sorted list, decode.
    P: the fz_scheme_params of hostpipe.scheme_params; L, R [N][d] key rows, pre [N][32] prehashes, c_hat [N][d], all in the
    callers' order; valid: [N] booleans, None = all.  order: sort_by_vk_string of ALL N keys when the caller has it (the sort
    is stable, so the valid signers' order is that order filtered).
    -> (order: caller indices of the valid signers in sorted order, alpha [N][d] coefficient rows in the callers' order, ZERO
    rows for the rest).  The aggregate and the target are sums over signers: with zero coefficients they are sums over the
    valid ones, so nothing has to be compacted or permuted on the device.  No device needed."""
    L = hostpipe._rows(L, P.degree)
    R = hostpipe._rows(R, P.degree)
    n = L.shape[0]
    alpha = np.zeros((n, P.degree), dtype=np.int32)
    if valid is None:
        keep = None
    else:
        keep = np.asarray(valid, dtype=bool).reshape(n)
        if keep.all():
            keep = None
    if order is None:
        if keep is None:
            order = hostpipe.sort_by_vk_string(P, L, R, threads)
        else:
            idx = np.flatnonzero(keep)
            order = idx[hostpipe.sort_by_vk_string(P, L[idx], R[idx], threads)] if idx.size else idx
    elif keep is not None:
        order = np.asarray(order)[keep[order]]
    if order.size:
        pre = np.ascontiguousarray(pre, dtype=np.uint8).reshape(-1, 32)
        c_hat = hostpipe._rows(c_hat, P.degree)
        alpha[order] = hostpipe.aggregation_coefficients(P, L[order], R[order], pre[order], c_hat[order], threads)
    return order, alpha


# ---- where the many-committee calls hash their aggregation coefficients (BatchScheme(hash_ag=...)) -------------------------
# "auto" predicts both forms from the committees' sizes.  A signer costs _HASH_AG_PERMS permutations either way (its ~10 KB of
# text absorbed, its section squeezed).  The device form is as long as its LONGEST committee's chain -- a wave's permutation takes
# _HASH_AG_DEVICE_US alone on its SIMD and _HASH_AG_SHARED more per further wave there (1024 SIMDs, up to four waves each: 4096
# committees in flight, then a second round) -- behind the ragged key sort, the upload of the pre-hashes and the launches.  The
# host form is the summed work over the scheme's threads at _HASH_AG_HOST_US per permutation and thread, behind what every
# committee costs the calling thread in Python.  All constants are medians of profiles/r25_hash_ag_many.txt (MI355X, 16
# threads), which also shows the rule picking the faster form in every cell it measures.
_HASH_AG_FORMS = ("host", "device", "auto")
_KEY_SORT_FORMS = ("host", "device")          # BatchScheme(key_sort=...): where the device form of hash_ag sorts each committee's keys
_HASH_AG_PERMS = {128: 30, 256: 99}           # per signer: (item text + section) / 136 (tools/probes/hash_ag_many.py)
_HASH_AG_SIMDS, _HASH_AG_WAVES = 1024, 4      # 256 CUs x 4 SIMDs; the kernel's waves per SIMD (127 registers, 26 KB LDS per workgroup)
_HASH_AG_DEVICE_US = 2.65                     # profiles/r25_hash_ag_many.txt: 64 x 64 at secpar 256, 16.81 ms / (64 x 99.2)
_HASH_AG_SHARED = 0.37                        # ... 4096 x 64: 35.7 ms, 2.1 times the lone wave's at four waves per SIMD
_HASH_AG_HOST_US = 0.2                        # ... 4096 x 64 against 4096 x 4 on the host: 0.15 (secpar 256) to 0.24 (128) per thread
_HASH_AG_HOST_COMMITTEE_US = 110.0            # ... 4096 x 4: 0.104 ms of the calling thread per committee (64 x 4: 0.10 to 0.15)
_HASH_AG_DEVICE_CALL_US = (500.0, 0.02)       # ... device - entry: 0.5 ms per call and 0.02 us per signer (sort, upload)


class BatchScheme:
    hash_ag = "host"                     # (the defaults of an object made without __init__)
    device_hash_ag = True
    key_sort = "host"

    def __init__(self, params, device=0, threads=None, private_context=False, hash_ag="host", key_sort="host"):
        """params: a fusion.fusion.Params (or any object with the same attributes).
        hash_ag: where the many-committee calls (aggregate_many, verify_many and their _encoded forms) hash the committees'
        aggregation coefficients: "host" (the default: one host thread per committee), "device" (one wave per committee,
        fz_hash_ag_ragged_dev: c_hat is not downloaded and the coefficients are not uploaded) or "auto" (the device form where
        it covers the parameter set and is predicted faster for the call's committee sizes).  The results are the same bit for
        bit; a parameter set the device form does not cover falls back to the host once and stays there.
        key_sort: where the DEVICE form of hash_ag sorts each committee's keys by str(vk): "host" (the default: one C call over a
        host copy of the keys, fz_sort_by_vk_string_ragged) or "device" (a wave per committee, fz_hash_ag_ragged_sorted_dev: keys
        that live on the device are not downloaded, the messages' digests stay on the device, and the call does not wait for
        either).  It has no effect where hash_ag takes its host form.  The results are the same bit for bit.
        private_context: give this object a context and a HIP stream of its own instead of the process-wide one per device.
        A context serves one host thread at a time (include/fusion_hip.h), so several BatchSchemes that are to work
        CONCURRENTLY -- one per worker thread -- each need their own.  That is how batches of the BASELINE size keep the chip
        busy: a 1024-signature sign_batch is a latency chain (108 Keccak permutations per signer on 32 waves: 0.63 of its
        0.87 ms) that leaves the other 250 CUs idle, and calls on separate streams overlap (tools/probes/concurrent_batches.py).
        close() releases the private context."""
        if hash_ag not in _HASH_AG_FORMS:
            raise FusionHipError(FZ_E_BADARG, f"hash_ag={hash_ag!r}: one of {_HASH_AG_FORMS}")
        if key_sort not in _KEY_SORT_FORMS:
            raise FusionHipError(FZ_E_BADARG, f"key_sort={key_sort!r}: one of {_KEY_SORT_FORMS}")
        self.params = params
        self.P = hostpipe.scheme_params(params)
        self.threads = threads or hostpipe.default_threads()
        self._pool = None
        self.d, self.l, self.q = params.degree, params.num_rows_sk, params.modulus
        self._private = bool(private_context)
        if self._private:
            self.ctx = Context(params.modulus, params.degree, params.root % params.modulus, params.inv_root % params.modulus, device)
            self._stream = self.ctx.stream_create()
            self.ctx.set_stream(self._stream)
        else:
            self.ctx = get_context(params.modulus, params.degree, params.root, params.inv_root, device)
        self.hash_ag = hash_ag           # where the many-committee calls hash their coefficients (_hash_ag_form)
        self.device_hash_ag = True       # ... its device form covers the parameter set (off after its first FZ_E_UNSUPPORTED)
        self.key_sort = key_sort         # ... and where that form sorts the committees' keys (_Committees.sort_dev)
        self.device_hash = True          # per-signer challenge pipeline on the device (falls back to the host if unsupported)
        self.device_sampler = True       # secret polynomials sampled on the device (the same fallback)
        self.A = np.array([z.values for row in params.public_challenge.matrix for z in row], dtype=np.int32)
        self._dA = None                  # the public challenge, resident on the device after its first use

    def _A_dev(self):
        if self._dA is None:
            self._dA = DeviceArray.from_numpy(self.ctx, self.A)
        return self._dA

    def close(self):
        """release the device copy of the public challenge, and the context if it is this object's own (the shared one stays)"""
        if self._dA is not None:
            self._dA.free()
            self._dA = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        if self._private and self.ctx is not None:
            self.ctx.set_stream(0)
            self.ctx.stream_destroy(self._stream)
            self.ctx.close()
            self.ctx = None

    # ---- device temporaries ------------------------------------------------------------------------------
    # Every method that allocates device memory does so inside ONE `with DeviceScope() as s`: what it uploads or allocates is
    # the scope's from the moment it exists and is freed on the way out, whatever raised; a result that stays on the device is
    # release()d to the caller.  Helpers that make buffers for their caller take that scope.
    def _dev(self, a, shape):
        """numpy array or DeviceArray -> (DeviceArray, owned?)"""
        if isinstance(a, DeviceArray):
            return a, False
        return DeviceArray.from_numpy(self.ctx, np.ascontiguousarray(a, dtype=np.int32).reshape(shape)), True

    def _take(self, scope, a, shape):
        """_dev into `scope`: an upload made here is the scope's, a caller's DeviceArray stays the caller's"""
        return a if isinstance(a, DeviceArray) else scope.own(self._dev(a, shape)[0])

    def _new(self, scope, shape, dtype=np.int32):
        return scope.own(DeviceArray(self.ctx, shape, dtype))

    def _up(self, scope, arr):
        return scope.own(DeviceArray.from_numpy(self.ctx, arr))

    def _records_dev(self, scope, data, n, rb):
        """the second half of _records_input: its n records [n][rb] on the device, uploaded into `scope` unless they are there"""
        return data if isinstance(data, DeviceArray) else self._up(scope, data.reshape(n, rb))

    @staticmethod
    def _check_dev(a, shape):
        if isinstance(a, DeviceArray) and (a.shape != shape or a.dtype != np.int32):
            raise FusionHipError(FZ_E_BADARG, f"device array {a.shape} {a.dtype}: {shape} int32 expected")

    # ---- keygen ------------------------------------------------------------------------------------
    def keygen_batch(self, seeds, device=False, keep_vk=False):
        """-> (sk_hat [N][2][l][d], vk [N][2][d]); key i equals keygen(params, seeds[i]).  With device=True
        sk_hat stays in device memory (a DeviceArray) -- vk always comes back (hash_ag hashes it on the host); with
        keep_vk=True a third value is returned, the verification keys as a DeviceArray [N][2][d] (what sign_batch's
        device challenge pipeline reads: pass it as `vk` and the keys are not uploaded again).
        Sampling: the reference draws every entry of a secret matrix with the SAME seed (fusion.py:156-173),
        so a matrix is one polynomial repeated l times; the polynomial itself comes from a clone of CPython's
        MT19937 `random` -- on the device (self.device_sampler) or in C on the host (hostpipe.sample_secret_polys); both
        are pinned against `random` in the tests.
        Unlike the reference this does not leave the process-global `random` generator re-seeded."""
        with DeviceScope() as s:
            return self._keygen_from_polys(s, self._sample_polys(s, seeds), device, keep_vk)

    def _sample_polys(self, s, seeds):
        """the secret polynomials [N][2][d] of `seeds`, by the sampler keygen_batch and keygen_batch_encoded share: a host array,
        or a DeviceArray owned by the scope `s` when the device sampler made them"""
        p = self.params
        # random.seed(int) uses abs(seed), so negative seeds are legal in the reference; the C / device samplers take the
        # non-negative seeds below 2^64 - 1
        # (keygen seeds the right half with seed + 1: for a negative seed that is abs(seed) - 1, not abs(seed) + 1)
        sd = _seed_array(seeds)
        # the reference's sampler yields ONE polynomial per (key, half) for all l rows (same seed for every matrix
        # entry): 2 KiB per key instead of 166 KiB.  Sampled on the device (an exact MT19937 per lane, fz_sample.hip) when
        # the parameter set allows (weight bound = degree), else by the C clone on the host threads and uploaded.
        polys = None
        if sd is None:
            polys = self._python_sampler(seeds)
        elif self.device_sampler:
            polys = self._new(s, (sd.size, 2, self.d))
            try:
                self.ctx.sample_secret_polys_dev(sd, p.modulus, p.degree, p.beta_sk, p.omega_sk, polys.ptr)
            except FusionHipError as e:
                if e.code != FZ_E_UNSUPPORTED:
                    raise
                self.device_sampler, polys = False, None
        if polys is None:
            polys = hostpipe.sample_secret_polys(sd, p.modulus, p.degree, p.beta_sk, p.omega_sk, self.threads)   # [N][2][d]
        return polys

    def keygen_batch_encoded(self, seeds, device=False, keep_vk=False):
        """keygen_batch straight to "secret" records: -> (records uint8 [N][encoded_size(params,
        "secret")], vk [N][2][d]); record i is bit for bit encode("secret", keygen_batch(seeds)[0])[0][i] (an honest key is
        within beta_sk: the codes are all 0, anything else raises FusionHipError(FZ_E_BADARG) that names the key).  With
        device=True the records stay on the device as a uint8 DeviceArray, which sign_batch_records takes as it is; with
        keep_vk=True a third value is returned, the verification keys as a DeviceArray [N][2][d], as keygen_batch does: pass it
        as `vk` to sign_batch_records and the keys are not uploaded again.  keygen_batch's sampler (the device sampler, its
        host clone, or the Python sampler for seeds the clones do not take), then ONE fused pass
        (keygen_records_async_dev, one polynomial per key half) that range-checks and packs the polynomials as it reads them
        and transforms them for the verification key alone: the int32 key [N][2][l][d] -- 4.57 times the record -- never
        exists on the device, and nothing is transformed back.
        Seeds that are not a flat sequence of integers raise FusionHipError(FZ_E_BADARG) before the device is touched.  No
        seeds: empty numpy arrays for either value of `device` (as sign_batch_records: a DeviceArray would need a device),
        the third value of keep_vk=True included."""
        _, _, bound, _, rb = _encoding(self.params, "secret")
        seeds = _integer_seeds(seeds)
        n = len(seeds)
        if n == 0:
            empty = np.zeros((0, rb), dtype=np.uint8), np.zeros((0, 2, self.d), dtype=np.int32)
            return empty + (np.zeros((0, 2, self.d), dtype=np.int32),) if keep_vk else empty
        with DeviceScope() as s:
            coef = self._take(s, self._sample_polys(s, seeds), (n, 2, self.d))
            dA = self._A_dev()
            dB, dK, dV = self._new(s, (n, rb), np.uint8), self._new(s, (n, 2, self.d)), self._new(s, (n,))
            self.ctx.keygen_records_async_dev(dA.ptr, coef.ptr, 1, n, self.l, bound, dB.ptr, dK.ptr, dV.ptr)
            codes = dV.numpy()
            if codes.any():
                bad = int(np.flatnonzero(codes)[0])
                raise FusionHipError(FZ_E_BADARG, f"key {bad}: {ENCODING_REASONS[int(codes[bad])]}")
            vk = dK.numpy()
            recs = s.release(dB) if device else dB.numpy()
            return (recs, vk, s.release(dK)) if keep_vk else (recs, vk)

    def _python_sampler(self, seeds):
        """the secret polynomials [N][2][d] for seeds the C / device MT19937 clones do not take (negative seeds, where seed + 1
        is not abs(seed) + 1, and seeds >= 2^64 - 1, whose keys have more words than the clones' two): from the drop-in's own
        sampler, i.e. CPython's `random` exactly as the reference drives it (polynomials.py:436-467)"""
        from algebra.polynomials import sample_polynomial_coefficient_representation as sample
        p = self.params
        polys = np.empty((len(seeds), 2, self.d), dtype=np.int32)
        for i, s in enumerate(seeds):
            for h in (0, 1):
                polys[i, h] = sample(modulus=p.modulus, degree=p.degree, root_order=p.root_order, root=p.root, inv_root=p.inv_root,
                                     norm_bound=p.beta_sk, weight_bound=p.omega_sk, seed=int(s) + h).coefficients
        return polys

    def _keygen_from_polys(self, s, polys, device, keep_vk):
        """keygen_batch after the sampling, the same for every sampler: polys [N][2][d], a host array or a DeviceArray of the
        caller's -> what keygen_batch returns; temporaries in the scope `s`"""
        n = polys.shape[0]
        coef = self._take(s, polys, (n, 2, self.d))
        dA = self._A_dev()
        sk, vk = self._new(s, (n, 2, self.l, self.d)), self._new(s, (n, 2, self.d))
        self.ctx.keygen_core_bcast_dev(dA.ptr, coef.ptr, sk.ptr, vk.ptr, n, self.l)
        vk_host = vk.numpy()
        res_sk = s.release(sk) if device else sk.numpy()
        return (res_sk, vk_host, s.release(vk)) if keep_vk else (res_sk, vk_host)

    # ---- sign --------------------------------------------------------------------------------------
    def challenges_dev(self, vk, messages, want_prehash=True, scope=None):
        """hash_ch for every (key, message) ON THE DEVICE (fz_challenge_hat_msgs_dev: SHA3-256 of the messages, text of
        str(vk), SHAKE-256, decoder, forward NTT): -> (c_hat DeviceArray [N][d], prehash [N][32] or None).  vk: numpy
        [N][2][d] or a DeviceArray of that shape.  Raises FusionHipError(FZ_E_UNSUPPORTED) for parameter sets the device
        pipeline does not cover.  c_hat is the caller's to free; with `scope` it is that DeviceScope's, as is an upload of vk."""
        if scope is None:
            with DeviceScope() as tmp:
                dC, pre = self.challenges_dev(vk, messages, want_prehash, tmp)
                return tmp.release(dC), pre
        blob, off = hostpipe._pack_messages(messages)
        n = len(messages)
        dV = self._take(scope, vk, (n, 2, self.d))
        dC = self._new(scope, (n, self.d))
        try:
            pre = self.ctx.challenge_msgs_dev(self.P, dV.ptr, blob, off, n, dC.ptr, want_prehash)
        finally:
            if dV is not vk:
                self.ctx.synchronize()                      # the launch has read the uploaded keys before they can go
        return dC, pre

    def challenges(self, vk, messages):
        """hash_ch for every (key, message): -> (c_hat [N][d], prehash [N][32]).  The per-signer pipeline runs on the
        device when it covers the parameter set (self.device_hash), else in the C host pipeline."""
        with DeviceScope() as s:
            return self._challenges_both(vk, messages, scope=s, want_dev=False)[1:]

    def sign_batch(self, sk_hat, vk, messages, device=False):
        """-> sig [N][l][d]; row i equals sign(params, key_i, messages[i]).signature_hat.
        sk_hat may be a numpy array or a DeviceArray; with device=True the signatures stay on the device.
        With the device challenge pipeline the challenges never visit the host."""
        with DeviceScope() as s:
            dC = self._challenges_both(vk, messages, want_host=False, scope=s)[0]
            n = dC.shape[0]
            dK = self._take(s, sk_hat, (n, 2, self.l, self.d))
            dS = self._new(s, (n, self.l, self.d))
            self.ctx.sign_core_dev(dK.ptr, dC.ptr, dS.ptr, n, self.l)
            if device:
                self.ctx.synchronize()
                return s.release(dS)
            return dS.numpy()

    def sign_batch_encoded(self, sk_hat, vk, messages, device=False):
        """sign_batch straight to the compact bytes: -> (data uint8 [N][encoded_size(params,
        "signature")], codes int32 [N]), bit for bit encode("signature", sign_batch(sk_hat, vk, messages)).  data is a numpy
        array, or with device=True a uint8 DeviceArray that aggregate_encoded / verify_signatures_encoded take as it is; codes
        are on the host: codes[i] is 4 (ENCODING_REASONS) when signature i is over the bound of one signature, and its bytes
        are then zero.  sk_hat [N][2][l][d] may be a numpy array or a DeviceArray.  The challenge pass is sign_batch's; one fused
        pass then signs, inverse-transforms, range-checks and packs: the int32 rows of the signatures (1.83 times the bytes
        the pass moves at secpar 256) never exist on the device.
        An sk_hat that is not [N][2][l][d] for N = the number of messages = the number of keys raises
        FusionHipError(FZ_E_BADARG) before the device is touched."""
        shape = tuple(sk_hat.shape if isinstance(sk_hat, DeviceArray) else np.shape(sk_hat))
        if len(shape) != 4 or shape[1:] != (2, self.l, self.d):
            raise FusionHipError(FZ_E_BADARG, f"sk_hat of shape {shape}: [N][2][{self.l}][{self.d}] expected")
        if isinstance(sk_hat, DeviceArray) and sk_hat.dtype != np.int32:
            raise FusionHipError(FZ_E_BADARG, f"device array of {sk_hat.dtype}: int32 expected")
        n = int(shape[0])
        return self._sign_to_bytes(n, "rows of sk_hat", vk, messages, device, lambda s: self._take(s, sk_hat, (n, 2, self.l, self.d)),
                                   lambda dK, dC, bound, dB, dV: self.ctx.sign_encoded_async_dev(dK, dC, n, self.l, bound, dB, dV))

    def sign_batch_records(self, secret, vk, messages, device=False):
        """sign_batch_encoded straight from the keys' compact bytes: `secret` holds N "secret" records
        in every form decode takes (bytes, bytearray, memoryview, a uint8 numpy array or a uint8 DeviceArray, e.g. what
        keygen_batch_encoded(device=True) returns) -> (data uint8 [N][encoded_size(params, "signature")], codes int32 [N]); for
        canonical records bit for bit sign_batch_encoded(decode("secret", secret)[0], vk, messages).  data is a numpy array, or
        with device=True a uint8 DeviceArray; codes are on the host: codes[i] is 6 (ENCODING_REASONS) when key record i is not
        canonical (a field above 2 beta_sk), and its bytes are then zero.  Code 4 cannot occur with hash_ch's challenges:
        |z| <= beta_sk (1 + omega_ch) = 1456 / 3172 <= signature_bound at secpar 128 / 256.  The challenge pass is sign_batch's;
        one fused pass then unpacks the key, transforms the left half, multiplies, transforms back, adds the right half,
        range-checks and packs: no int32 row of key or signature exists on the device.
        A length that is not N whole records, or a number of keys or messages other than N, raises
        FusionHipError(FZ_E_BADARG) before the device is touched.  N == 0 returns empty numpy arrays for either value of
        `device`, as sign_batch_encoded does: the call then needs no device, which a DeviceArray would (decode, which is
        given its device by the caller's choice of `device`, returns an empty DeviceArray there)."""
        _, _, key_bound, _, kb = _encoding(self.params, "secret")
        secret, n = _records_input("secret", secret, kb)
        return self._sign_to_bytes(n, "secret records", vk, messages, device, lambda s: self._records_dev(s, secret, n, kb),
                                   lambda dK, dC, bound, dB, dV: self.ctx.sign_records_async_dev(dK, key_bound, dC, n, self.l, bound, dB, dV))

    def _vk_of_records(self, s, dK, n):
        """the verification keys of the n "secret" records dK holds on the device, in one pass (vk_records_async_dev): -> (a
        DeviceArray [n][2][d] of the scope `s`, codes int32 [n] on the host: 0, or 6 with the key's vk zero)"""
        key_bound = _encoding(self.params, "secret")[2]
        dV, dS = self._new(s, (n, 2, self.d)), self._new(s, (n,))
        self.ctx.vk_records_async_dev(self._A_dev().ptr, dK.ptr, key_bound, n, self.l, dV.ptr, dS.ptr)
        return dV, dS.numpy()

    def vk_from_records(self, secret, device=False):
        """the verification keys of N "secret" records (`secret` in every form decode takes) -> (vk
        [N][2][d], codes int32 [N]): vk[i] is bit for bit the key keygen_batch_encoded returned beside record i, and
        matvec(A, decode("secret", secret)[0]) for any canonical record.  vk is a numpy array, or with device=True a DeviceArray
        that challenges_dev / sign_batch_records take as it is; codes are on the host: codes[i] is 6 (ENCODING_REASONS) when
        record i is not canonical (a field above 2 beta_sk), and vk[i] is then zero.  One fused pass unpacks, range-checks and
        transforms the key and multiplies by the public challenge: the int32 key [N][2][l][d] -- 4.57 times the record -- never
        exists on the device.
        A length that is not N whole records raises FusionHipError(FZ_E_BADARG) before the device is touched.  N == 0 returns
        empty numpy arrays for either value of `device`, as sign_batch_records does."""
        kb = _encoding(self.params, "secret")[4]
        secret, n = _records_input("secret", secret, kb)
        if n == 0:
            return np.zeros((0, 2, self.d), dtype=np.int32), np.zeros(0, dtype=np.int32)
        with DeviceScope() as s:
            dV, codes = self._vk_of_records(s, self._records_dev(s, secret, n, kb), n)
            return (s.release(dV) if device else dV.numpy()), codes

    def sign_batch_secret(self, secret, messages, device=False):
        """sign_batch_records from the records alone: -> (data uint8 [N][encoded_size(params, "signature")], codes int32 [N], vk
        [N][2][d] int32).  The keys are derived on the device (vk_from_records' pass), sign_batch's challenge pass reads them
        where they are -- no key is uploaded -- and one sign_records_async_dev launch signs; for canonical records data and
        codes are bit for bit sign_batch_records(secret, vk, messages).  data is a numpy array, or with device=True a uint8
        DeviceArray; codes and vk are on the host (aggregate needs the keys there).  A record with code 6 signs nothing: its
        bytes are zero, and so is its vk.
        A length that is not N whole records, or a number of messages other than N, raises FusionHipError(FZ_E_BADARG) before
        the device is touched.  N == 0 returns empty numpy arrays for either value of `device`."""
        _, _, key_bound, _, kb = _encoding(self.params, "secret")
        _, _, bound, _, rb = _encoding(self.params, "signature")
        secret, n = _records_input("secret", secret, kb)
        if len(messages) != n:
            raise FusionHipError(FZ_E_BADARG, f"{len(messages)} messages, {n} secret records")
        if n == 0:
            return np.zeros((0, rb), dtype=np.uint8), np.zeros(0, dtype=np.int32), np.zeros((0, 2, self.d), dtype=np.int32)
        with DeviceScope() as s:
            dK = self._records_dev(s, secret, n, kb)
            dV = self._vk_of_records(s, dK, n)[0]           # (a record refused here is refused by the signing pass too)
            dC = self._challenges_both(dV, messages, want_host=False, scope=s)[0]
            dB, dS = self._new(s, (n, rb), np.uint8), self._new(s, (n,))
            self.ctx.sign_records_async_dev(dK.ptr, key_bound, dC.ptr, n, self.l, bound, dB.ptr, dS.ptr)
            codes, vk = dS.numpy(), dV.numpy()
            return (s.release(dB) if device else dB.numpy()), codes, vk

    def check_keypairs(self, secret, vk):
        """does "secret" record i belong to vk[i]?  -> codes int32 [N]: 0 when the record is canonical and its derived key
        (vk_from_records) equals vk[i] mod q, 3 (VERDICT_REASONS: the target mismatch) when it does not, 6 (ENCODING_REASONS)
        when the record is not canonical.  vk [N][2][d]: a numpy array or a DeviceArray, any residues.  The keys are derived
        on the device and compared on the host (2 KiB per key).
        A length that is not N whole records, or a number of keys other than N, raises FusionHipError(FZ_E_BADARG) before
        the device is touched."""
        kb = _encoding(self.params, "secret")[4]
        secret, n = _records_input("secret", secret, kb)
        try:
            nk = self._signer_count(vk)
        except ValueError:
            nk = -1
        if nk != n:
            raise FusionHipError(FZ_E_BADARG, f"{nk} keys, {n} secret records")
        if n == 0:
            return np.zeros(0, dtype=np.int32)
        derived, codes = self.vk_from_records(secret)
        want = self._split_vk(vk)[0]
        same = ((derived.astype(np.int64) - want.astype(np.int64)) % self.q == 0).all(axis=(1, 2))
        return np.where(codes != 0, codes, np.where(same, 0, 3)).astype(np.int32)

    def _sign_to_bytes(self, n, keys_are, vk, messages, device, key_dev, launch):
        """what sign_batch_encoded and sign_batch_records share once the key's own checks gave its N = n (`keys_are`: what n counts,
        for the message): the count check, the empty answer, and in one DeviceScope the challenges, the key on the device
        (key_dev(scope)), the output and status buffers, launch(key, challenges, bound, bytes, status), the codes, and the
        bytes released or downloaded"""
        _, _, bound, _, rb = _encoding(self.params, "signature")
        try:
            nk = self._signer_count(vk)
        except ValueError:
            nk = -1
        if not (nk == len(messages) == n):
            raise FusionHipError(FZ_E_BADARG, f"{nk} keys, {len(messages)} messages, {n} {keys_are}")
        if n == 0:
            return np.zeros((0, rb), dtype=np.uint8), np.zeros(0, dtype=np.int32)
        with DeviceScope() as s:
            dC = self._challenges_both(vk, messages, want_host=False, scope=s)[0]
            dK = key_dev(s)
            dB, dV = self._new(s, (n, rb), np.uint8), self._new(s, (n,))
            launch(dK.ptr, dC.ptr, bound, dB.ptr, dV.ptr)
            codes = dV.numpy()
            return (s.release(dB) if device else dB.numpy()), codes

    # ---- aggregate / verify ----------------------------------------------------------------------------
    def _split_vk(self, vk):
        vk = np.ascontiguousarray(vk.numpy() if isinstance(vk, DeviceArray) else vk, dtype=np.int32).reshape(-1, 2, self.d)
        return vk, np.ascontiguousarray(vk[:, 0]), np.ascontiguousarray(vk[:, 1])

    def _signer_count(self, vk):
        return vk.shape[0] if isinstance(vk, DeviceArray) else np.asarray(vk).reshape(-1, 2, self.d).shape[0]

    def _challenges_both(self, vk, messages, want_host=True, scope=None, want_dev=True, want_pre=None):
        """hash_ch for every (key, message) in the CALLERS' order: -> (dC DeviceArray [N][d], c_hat host copy, prehash
        [N][32]).  THE place of the rule "the device pipeline where it covers the parameter set, else the C host pipeline"
        (FZ_E_UNSUPPORTED from the device once, and self.device_hash stays off).  The device pipeline leaves c_hat where the
        kernels need it; hash_ag needs a host copy of it as text input (want_host=False, no hash_ag behind the call: the
        device pipeline downloads neither, None for both).  want_dev=False (challenges()): nothing stays on the device, None
        for dC, and the host pipeline uploads nothing.  want_pre (default: want_host): the prehashes without the host copy of
        c_hat, for the device form of hash_ag.  dC is the caller's to free (dist.HipSteps), or with `scope` that DeviceScope's."""
        want_pre = want_host if want_pre is None else want_pre
        if scope is None:
            with DeviceScope() as tmp:
                dC, c_hat, pre = self._challenges_both(vk, messages, want_host, tmp, want_dev, want_pre)
                return (tmp.release(dC) if want_dev else None), c_hat, pre
        if self.device_hash:
            try:
                dC, pre = self.challenges_dev(vk, messages, want_pre, scope)
                return (dC if want_dev else None), (dC.numpy() if want_host else None), pre
            except FusionHipError as e:
                if e.code != FZ_E_UNSUPPORTED:
                    raise
                self.device_hash = False
        _, L, R = self._split_vk(vk)
        coefs, pre = hostpipe.challenge_coefficients(self.P, L, R, messages, self.threads)
        c_hat = self.ctx.ntt_forward(coefs)
        return (self._up(scope, c_hat) if want_dev else None), c_hat, pre

    def _sort_async(self, L, R):
        """sort_by_vk_string on a worker thread (the C call releases the GIL): it needs only the keys, so it runs beside the
        device challenge pipeline instead of after it; -> a future of the order"""
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="fz-sort")
        return self._pool.submit(hostpipe.sort_by_vk_string, self.P, L, R, self.threads)

    def _alpha_coefficients(self, L, R, pre, c_hat, threads=None, order=None):
        """hash_ag without the transforms (fusion.py:632-652) for ONE aggregate: sort by str(vk) (fusion.py:661-663, :693), the
        one serial SHAKE-256 over the sorted list, decode; -> (order, alpha coefficient rows scattered back to the CALLERS'
        order).  The aggregate and the target are sums over signers, so nothing else ever has to be permuted."""
        return screened_alpha_coefficients(self.P, L, R, pre, c_hat, None, threads or self.threads, order)

    def _alpha_hat(self, scope, alpha):
        """coefficient rows [N][d] -> alpha_hat in `scope`: one upload, the forward transform in place (a zero row stays zero)"""
        dAl = self._up(scope, alpha)
        self.ctx.ntt_forward_dev(dAl.ptr, dAl.ptr, alpha.shape[0])
        return dAl

    def _aggregate_valid(self, scope, valid, L, R, pre, c_hat, order, sig=None, encoded=None):
        """the shared tail of the screened aggregations: hash_ag over the signers with valid[i] set (zero coefficient rows for the
        rest, so nothing is compacted), upload, forward transform in place, one aggregation launch, download: -> aggregate [l][d].
        From the rows `sig` [N][l][d], or from encoded = (dB, dV): the "signature" records on the device and its own verdict
        words, nonzero for the rest, which the fused pass takes as they are for its skip words: a rejected record is not read."""
        _, alpha = screened_alpha_coefficients(self.P, L, R, pre, c_hat, valid, self.threads, order)
        n = alpha.shape[0]
        dO, dAl = self._new(scope, (self.l, self.d)), self._alpha_hat(scope, alpha)
        if encoded is None:
            dS = self._take(scope, sig, (n, self.l, self.d))
            self.ctx.aggregate_core_dev(dS.ptr, dAl.ptr, dO.ptr, n, self.l)
        else:
            dP = self._new(scope, (self.l, self.d), np.int64)
            bound = _encoding(self.params, "signature")[2]
            self.ctx.aggregate_encoded_async_dev(encoded[0].ptr, dAl.ptr, encoded[1].ptr, n, self.l, bound, dP.ptr, dO.ptr)
        return dO.numpy()

    def _hash_ag_host(self, vk, messages, scope, keep_c=True):
        """the keys' and messages' share of one hash_ag, with the key sort on its worker beside the challenge pass (neither
        needs the other): -> (dC, c_hat, pre, order, L, R); keep_c=False: c_hat does not stay on the device, None for dC"""
        vk, L, R = self._split_vk(vk)
        order_f = self._sort_async(L, R)
        try:
            with DeviceScope() as tmp:                      # keep_c=False: c_hat leaves the device once its host copy is here
                dC, c_hat, pre = self._challenges_both(vk, messages, scope=scope if keep_c else tmp)
        finally:
            order = order_f.result()
        return (dC if keep_c else None), c_hat, pre, order, L, R

    def hash_ag_dev(self, vk, messages, scope=None):
        """Everything aggregate() and verify() derive from the keys and messages, device-resident and in the callers' order:
        -> (dC [N][d] challenges c_hat, dAl [N][d] aggregation coefficients alpha_hat, order, vkL, vkR host rows).  dC and dAl
        are the caller's to free, or with `scope` that DeviceScope's."""
        if scope is None:
            with DeviceScope() as tmp:
                dC, dAl, order, L, R = self.hash_ag_dev(vk, messages, tmp)
                return tmp.release(dC), tmp.release(dAl), order, L, R
        dC, c_hat, pre, order, L, R = self._hash_ag_host(vk, messages, scope)
        order, alpha = self._alpha_coefficients(L, R, pre, c_hat, order=order)
        return dC, self._alpha_hat(scope, alpha), order, L, R

    def aggregate(self, vk, messages, sig):
        """-> aggregate [l][d] == aggregate(params, keys, messages, signatures).signature_hat.
        sig may be a numpy array or a DeviceArray.  Challenges and aggregation coefficients stay on the device; only the
        keys' text input of hash_ag and the result cross PCIe."""
        with DeviceScope() as s:
            dC, dAl, _, _, _ = self.hash_ag_dev(vk, messages, scope=s)
            n = dAl.shape[0]
            dS = self._take(s, sig, (n, self.l, self.d))
            dO = self._new(s, (self.l, self.d))
            self.ctx.aggregate_core_dev(dS.ptr, dAl.ptr, dO.ptr, n, self.l)
            return dO.numpy()

    def aggregate_verify(self, vk, messages, sig):
        """aggregate() followed by verify() of the result on the same keys and messages, as an aggregator that checks its own
        output does: -> (aggregate [l][d], (ok, reason)).  hash_ag -- the one serial SHAKE-256 over all signers that bounds both
        calls end to end -- runs ONCE instead of twice, the signatures are read once (aggregate and verification target in one
        pass), and the verdict comes straight from the int64 sums.  Same values as aggregate(...) and verify(..., aggregate)."""
        from .dist import LocalCollective, ShardedScheme
        return ShardedScheme(self, 0, 1, LocalCollective(self.ctx)).aggregate_verify_sharded(vk, messages, sig)

    # ---- the steps the four verify forms share ------------------------------------------------------------
    def _refused(self, n, messages):
        """the verdicts that need no arithmetic, capacity first (fusion.py:686-689): -> (False, reason), or None to go on"""
        if n > self.params.capacity:
            return False, VERDICT_REASONS[1]
        if n != len(messages):
            return False, VERDICT_REASONS[2]
        return None

    def _one_by_one(self, single, vk, messages, items, shape, sizes):
        """verify_many / verify_many_encoded when some group is over capacity (rare; it keeps the batch path simple): that
        group's verdict is the capacity one, the others are verified one by one by single(vk_g, messages_g, items_g);
        -> the verdicts, or None when every group is within capacity"""
        live = [i for i, n in enumerate(sizes) if n <= self.params.capacity]
        if len(live) == len(sizes):
            return None
        out = [(False, VERDICT_REASONS[1])] * len(sizes)
        vkh, _, _ = self._split_vk(vk)
        off = np.concatenate([[0], np.cumsum(sizes)])
        items = (items.numpy() if isinstance(items, DeviceArray) else np.asarray(items)).reshape((len(sizes),) + shape)
        for i in live:
            out[i] = single(vkh[off[i]:off[i + 1]], messages[off[i]:off[i + 1]], items[i])
        return out

    def _target(self, scope, dL, dR, dC, dAl, n):
        """the verification target of ONE aggregate of n signers, centred: -> dT [d]"""
        dT64, dT = self._new(scope, (self.d,), np.int64), self._new(scope, (self.d,))
        self.ctx.target_partial_dev(dL.ptr, dR.ptr, dC.ptr, dAl.ptr, dT64.ptr, n)
        self.ctx.reduce_i64_dev(dT64.ptr, dT.ptr, self.d)
        return dT

    def _targets(self, scope, dL, dR, dC, dAl, off):
        """the verification targets of the len(off) - 1 aggregates of rows off[g]:off[g+1], one launch, centred: -> dT [G][d]"""
        g = len(off) - 1
        dT64, dT = self._new(scope, (g, self.d), np.int64), self._new(scope, (g, self.d))
        self.ctx.aggregate_target_partial_ragged_dev(0, dAl.ptr, dL.ptr, dR.ptr, dC.ptr, off, self.l, 0, 0, dT64.ptr, self.d)
        self.ctx.reduce_i64_dev(dT64.ptr, dT.ptr, g * self.d)
        return dT

    def verify(self, vk, messages, aggregate):
        """-> (bool, reason) with the reference's reason strings (fusion.py:680-728)"""
        n = self._signer_count(vk)
        refused = self._refused(n, messages)
        if refused is not None:
            return refused
        with DeviceScope() as s:
            dC, dAl, _, L, R = self.hash_ag_dev(vk, messages, scope=s)
            dL, dR = self._up(s, L), self._up(s, R)
            dS = self._take(s, aggregate, (self.l, self.d))
            return _verdict(self.ctx.verify_core_dev(self._A_dev().ptr, dS.ptr, dL.ptr, dR.ptr, dC.ptr, dAl.ptr, n, self.l,
                                                     int(self.params.beta_vf), int(self.params.omega_vf)))

    # ---- one signature at a time (not in the reference) ----------------------------------------------------
    def _screen(self, vk, messages, sig, beta, omega, want_hash_ag, scope):
        """the per-signature verdicts of N signers, -> (codes [N] int32, c_hat host copy, prehash), the last two None unless
        want_hash_ag.  One challenge pass, one launch, one verdict download; vk is uploaded once (the challenge pipeline reads
        the same copy)."""
        n = self._signer_count(vk)
        if n != len(messages):
            raise FusionHipError(FZ_E_BADARG, f"{n} keys but {len(messages)} messages")
        beta = signature_bound(self.params) if beta is None else int(beta)
        omega = int(self.params.omega_vf) if omega is None else int(omega)
        if beta < 0 or omega < 0:
            raise FusionHipError(FZ_E_BADARG, f"bounds must be non-negative (beta={beta}, omega={omega})")
        self._check_dev(vk, (n, 2, self.d))
        self._check_dev(sig, (n, self.l, self.d))
        if n == 0:
            return np.zeros(0, dtype=np.int32), None, None
        dK = self._take(scope, vk, (n, 2, self.d))
        dC, c_hat, pre = self._challenges_both(dK, messages, want_hash_ag, scope=scope)
        dS = self._take(scope, sig, (n, self.l, self.d))
        dV = self._new(scope, (n,))
        self.ctx.verify_signatures_async_dev(self._A_dev().ptr, dS.ptr, dK.ptr, dC.ptr, n, self.l, beta, omega, dV.ptr)
        return (dV.numpy(), c_hat, pre) if want_hash_ag else (dV.numpy(), None, None)

    def verify_signatures(self, vk, messages, sig, beta=None, omega=None):
        """Per-signature verification (not a reference function): -> int32 codes [N], 0 where signer i's signature is valid
        for (vk[i], messages[i]), else the first failing check (SIGNATURE_REASONS): 3 when A (.) sig_i != vkL_i (.) c_i + vkR_i,
        4 when ||INTT(sig_i)||_inf > beta, 5 when a row's weight > omega.  That is verify() of the aggregate of one signer with
        alpha_hat == 1, against the bound of ONE signature: beta defaults to signature_bound(params) (4264 at secpar 128,
        3172 at 256; a params object of another secpar must pass it), omega to params.omega_vf.  vk [N][2][d] and sig
        [N][l][d] may be numpy arrays or DeviceArrays (keygen_batch(..., keep_vk=True) / sign_batch(..., device=True)).
        Unequal numbers of keys and messages raise FusionHipError(FZ_E_BADARG): a caller error, not a verdict."""
        with DeviceScope() as s:
            return self._screen(vk, messages, sig, beta, omega, False, s)[0]

    def aggregate_screened(self, vk, messages, sig):
        """aggregate() over the signers whose signature passes verify_signatures, for aggregators that take untrusted
        contributions: -> (aggregate [l][d] or None when no signer passes, codes [N]).  The aggregate is bit for bit
        aggregate(vk[ok], messages[ok], sig[ok]) -- one bad contribution no longer spoils the aggregate, and the codes say
        whose it was.  One challenge pass serves both steps; hash_ag runs over the valid signers only, its coefficients are
        scattered back with zero rows for the rejected ones, so the signature rows are never compacted."""
        with DeviceScope() as s:                            # of its own: the screen's copy of sig goes before the aggregation's comes
            codes, c_hat, pre = self._screen(vk, messages, sig, None, None, True, s)
        valid = codes == 0
        if not valid.any():
            return None, codes
        _, L, R = self._split_vk(vk)
        with DeviceScope() as s:
            return self._aggregate_valid(s, valid, L, R, pre, c_hat, None, sig=sig), codes

    # ---- compact byte encoding (not in the reference) ------------------------------------
    def encode(self, kind, rows):
        """-> (data uint8 [N][encoded_size(params, kind)], codes int32 [N]): the canonical bytes of N keys ("vk", rows
        [N][2][d]), signatures or aggregates ("signature" / "aggregate", rows [N][l][d]; one [l][d] aggregate is N = 1), as
        numpy arrays or a DeviceArray.  codes[i] is 4 (ENCODING_REASONS) when record i is over its kind's bound -- exactly the
        signatures verify_signatures rejects for the norm, the aggregates verify() rejects for it; keys never are -- and its
        bytes are then zero.  "secret": the signing keys sk_hat [N][2][l][d] (or [N][2l][d]), left half first, under beta_sk;
        code 4 means a key the reference's keygen cannot make."""
        nrows, coef, bound, w, rb = _encoding(self.params, kind)
        shape = rows.shape if isinstance(rows, DeviceArray) else np.shape(rows)
        if kind == "secret" and len(shape) == 4 and tuple(shape[1:]) == (2, self.l, self.d):
            shape = (shape[0], nrows, self.d)
        elif kind not in ("vk", "secret") and len(shape) == 2:
            shape = (1,) + tuple(shape)
        if len(shape) != 3 or tuple(shape[1:]) != (nrows, self.d):
            raise FusionHipError(FZ_E_BADARG, f"rows of shape {tuple(shape)}: [N][{nrows}][{self.d}] expected for {kind!r}")
        if isinstance(rows, DeviceArray) and rows.dtype != np.int32:
            raise FusionHipError(FZ_E_BADARG, f"device array of {rows.dtype}: int32 expected")
        n = int(shape[0])
        if n == 0:
            return np.zeros((0, rb), dtype=np.uint8), np.zeros(0, dtype=np.int32)
        with DeviceScope() as s:
            dR = self._take(s, rows, (n, nrows, self.d))
            dB, dV = self._new(s, (n, rb), np.uint8), self._new(s, (n,))
            self.ctx.encode_records_async_dev(dR.ptr, n, nrows, coef, bound, dB.ptr, dV.ptr)
            return dB.numpy(), dV.numpy()

    def decode(self, kind, data, device=False):
        """-> (rows, codes int32 [N]): the records of `data` (bytes, bytearray, memoryview, a uint8 numpy array or a uint8
        DeviceArray; N * encoded_size(params, kind) bytes) as int32 rows [N][2][d] ("vk"), [N][2][l][d] ("secret") or [N][l][d],
        NTT domain, centred -- numpy, or a DeviceArray with device=True (straight into verify_signatures / aggregate).
        codes[i] is 6 (ENCODING_REASONS) when record i is not canonical (a field above 2B), and its rows are then zero.  A
        length that is not a whole number of records raises FusionHipError(FZ_E_BADARG)."""
        nrows, coef, bound, w, rb = _encoding(self.params, kind)
        data, n = _records_input(kind, data, rb)
        shape = (2, self.l, self.d) if kind == "secret" else (nrows, self.d)
        if n == 0:
            empty = np.zeros((0,) + shape, dtype=np.int32)
            return (DeviceArray.from_numpy(self.ctx, empty) if device else empty), np.zeros(0, dtype=np.int32)
        with DeviceScope() as s:
            dB = self._records_dev(s, data, n, rb)
            dR, dV = self._new(s, (n,) + shape), self._new(s, (n,))
            self.ctx.decode_records_async_dev(dB.ptr, n, nrows, coef, bound, dR.ptr, dV.ptr)
            codes = dV.numpy()
            return (s.release(dR) if device else dR.numpy()), codes

    def _signature_records(self, vk, messages, data):
        """the byte input of the calls that take one "signature" record per signer, refused with FusionHipError(FZ_E_BADARG)
        unless it is whole records and as many as there are keys and messages: -> (nrows, bound, rb, data, n)"""
        nrows, _, bound, _, rb = _encoding(self.params, "signature")
        data, n = _records_input("signature", data, rb)
        nk = self._signer_count(vk)
        if not (nk == len(messages) == n):
            raise FusionHipError(FZ_E_BADARG, f"{nk} keys, {len(messages)} messages, {n} records")
        return nrows, bound, rb, data, n

    def aggregate_encoded(self, vk, messages, data):
        """aggregate() straight from the signatures' compact bytes (`data`: N "signature" records in every form decode
        takes): -> (aggregate [l][d] int32, or None when no record is canonical; codes int32 [N]).  codes[i] is 0, or 6
        (ENCODING_REASONS) when record i is not canonical (a field above 2B); the aggregate is bit for bit
        aggregate(vk[ok], messages[ok], decode("signature", data)[0][ok]) over the records with code 0 -- hash_ag runs over
        those signers only, as aggregate_screened does.  The bytes are uploaded once, range-checked (beside the challenge pass
        and the key sort), and one fused pass unpacks, transforms, multiplies and accumulates them: the int32 rows of the
        signatures (2.46 times the bytes at secpar 256) never exist on the device.
        What this call does NOT do: a canonical record is within the norm bound of ONE signature, but its target equation
        A (.) sig_i == vkL_i (.) c_i + vkR_i is not checked.  An aggregator of mostly honest input verifies its own aggregate
        (aggregate_verify_encoded does both in one pass; verify afterwards repeats the challenge pass and hash_ag); when that
        fails, aggregate_encoded_screened on the same bytes names the signer.
        A length that is not N whole records, or numbers of keys / messages other than N, raise FusionHipError(FZ_E_BADARG)
        before the device is touched."""
        nrows, bound, rb, data, n = self._signature_records(vk, messages, data)
        if n == 0:
            return None, np.zeros(0, dtype=np.int32)
        with DeviceScope() as s:
            dB = self._records_dev(s, data, n, rb)
            dV = self._new(s, (n,))
            self.ctx.check_records_async_dev(dB.ptr, n, nrows, bound, dV.ptr)
            # beside the check; hash_ag reads the host copy of c_hat, nothing here needs it on the device
            _, c_hat, pre, order, L, R = self._hash_ag_host(vk, messages, s, keep_c=False)
            codes = dV.numpy()
            valid = codes == 0
            if not valid.any():
                return None, codes
            return self._aggregate_valid(s, valid, L, R, pre, c_hat, order, encoded=(dB, dV)), codes

    # ---- verification straight from the bytes (not in the reference) ---------------------
    def _screen_encoded(self, vk, messages, data, aggregate):
        """verify_signatures_encoded, and with aggregate=True the screened aggregation behind it: -> (aggregate or None,
        codes).  The argument checks come before anything touches the device."""
        _, bound, rb, data, n = self._signature_records(vk, messages, data)
        self._check_dev(vk, (n, 2, self.d))
        if n == 0:
            return None, np.zeros(0, dtype=np.int32)
        with DeviceScope() as s:
            dB = self._records_dev(s, data, n, rb)
            dK = self._take(s, vk, (n, 2, self.d))
            dV = self._new(s, (n,))
            dC, c_hat, pre = self._challenges_both(dK, messages, aggregate, scope=s)
            self.ctx.verify_encoded_async_dev(self._A_dev().ptr, dB.ptr, n, self.l, bound, 0, dK.ptr, dC.ptr, dV.ptr)
            codes = dV.numpy()
            valid = codes == 0
            if not aggregate or not valid.any():
                return None, codes
            _, L, R = self._split_vk(vk)
            return self._aggregate_valid(s, valid, L, R, pre, c_hat, None, encoded=(dB, dV)), codes

    def verify_signatures_encoded(self, vk, messages, data):
        """verify_signatures straight from the signatures' compact bytes (`data`: N "signature" records in every form decode
        takes; vk [N][2][d] numpy or DeviceArray): -> int32 codes [N].  codes[i] is 6 (ENCODING_REASONS) when record i is not
        canonical (a field above 2B) -- it then has no value to test, so this comes first --, else 3 (SIGNATURE_REASONS) when
        A (.) sig_i != vkL_i (.) c_i + vkR_i, else 0.  Codes 4 and 5 cannot occur: a canonical record is within the bound of
        one signature by construction, and the weight bound omega_vf = d cannot fail.  For canonical records the codes equal
        verify_signatures(vk, messages, decode("signature", data)[0]).  One upload of the bytes, one challenge pass, one launch,
        one verdict download; the int32 rows of the signatures never exist on the device.  A length that is not N whole records,
        or numbers of keys / messages other than N, raise FusionHipError(FZ_E_BADARG) before the device is touched."""
        return self._screen_encoded(vk, messages, data, False)[1]

    def aggregate_encoded_screened(self, vk, messages, data):
        """aggregate_screened straight from the bytes: -> (aggregate [l][d] or None when no signer passes, codes [N] of
        verify_signatures_encoded).  The verdict words stay on the device and are the skip words of the fused aggregation, so
        a rejected record is not read a second time; hash_ag runs over the signers with code 0 only.  The aggregate is bit
        for bit aggregate_screened(vk, messages, decode("signature", data)[0])[0]: a record that is not canonical (code 6
        here) decodes to zero rows, which that call rejects as well."""
        return self._screen_encoded(vk, messages, data, True)

    def verify_encoded(self, vk, messages, data):
        """verify() of an aggregate given as ONE "aggregate" record (every form decode takes): -> (bool, reason), equal to
        verify(vk, messages, decode("aggregate", data)[0][0]) for a canonical record; a record that is not canonical gives
        (False, ENCODING_REASONS[6]).  The aggregate's int32 rows never exist on the device.  Anything but exactly one whole
        record raises FusionHipError(FZ_E_BADARG) before the device is touched."""
        _, _, bound, _, rb = _encoding(self.params, "aggregate")
        data, nrec = _records_input("aggregate", data, rb)
        if nrec != 1:
            raise FusionHipError(FZ_E_BADARG, f"{nrec} 'aggregate' records: exactly one expected")
        n = self._signer_count(vk)
        refused = self._refused(n, messages)
        if refused is not None:
            return refused
        with DeviceScope() as s:
            dC, dAl, _, L, R = self.hash_ag_dev(vk, messages, scope=s)
            dL, dR = self._up(s, L), self._up(s, R)
            dB = self._records_dev(s, data, 1, rb)
            dV, dT = self._new(s, (1,)), self._target(s, dL, dR, dC, dAl, n)
            self.ctx.verify_encoded_async_dev(self._A_dev().ptr, dB.ptr, 1, self.l, bound, dT.ptr, 0, 0, dV.ptr)
            return _verdict(dV.numpy()[0])

    # ---- many aggregates at once ------------------------------------------------------------------------
    def _many_sizes(self, vk, messages, sizes):
        """sizes as ints, refused with FusionHipError(FZ_E_BADARG) unless each is at least 1 and they sum to the numbers of keys and
        of messages; no device is touched"""
        sizes = [int(x) for x in sizes]
        if any(x < 1 for x in sizes):
            raise FusionHipError(FZ_E_BADARG, "every aggregate needs at least one signer")
        nk = self._signer_count(vk)
        if not (sum(sizes) == nk == len(messages)):
            raise FusionHipError(FZ_E_BADARG, f"sizes sum to {sum(sizes)} but {nk} keys and {len(messages)} messages were given")
        return sizes

    def _hash_ag_form(self, sizes):
        """"host" or "device": where a many-committee call over committees of `sizes` hashes its coefficients (self.hash_ag; the
        rule of "auto" and its constants: _HASH_AG_* above)"""
        if self.hash_ag == "host" or not self.device_hash_ag or not len(sizes):
            return "host"
        if self.hash_ag == "device":
            return "device"
        perms = _HASH_AG_PERMS.get(getattr(self.params, "secpar", None), 99)
        g, n = len(sizes), sum(sizes)
        resident = _HASH_AG_SIMDS * _HASH_AG_WAVES
        sharing = min(_HASH_AG_WAVES, -(-g // _HASH_AG_SIMDS)) - 1
        chain = max(sizes) * perms * _HASH_AG_DEVICE_US * (1 + _HASH_AG_SHARED * sharing)
        device = _HASH_AG_DEVICE_CALL_US[0] + _HASH_AG_DEVICE_CALL_US[1] * n + -(-g // resident) * chain
        host = g * _HASH_AG_HOST_COMMITTEE_US + n * perms * _HASH_AG_HOST_US / max(1, min(self.threads, g))
        return "device" if device < host else "host"

    def sort_keys_many_dev(self, vk, sizes, valid=None):
        """the order in which hash_ag hashes the keys of G committees (sizes = keys per committee, concatenated), computed ON THE
        DEVICE (fz_sort_by_vk_string_ragged_dev, a wave per committee): -> int64 row indices into vk [sum N][2][d] (numpy or
        DeviceArray), committee after committee, each committee's rows with valid[i] set (None: all) in the order
        sorted(key=str) puts their keys -- hostpipe.sort_by_vk_string_ragged's order, filtered."""
        sizes = [int(x) for x in sizes]
        off = _offsets(sizes)
        n = int(off[-1])
        if any(x < 0 for x in sizes) or n != self._signer_count(vk):
            raise FusionHipError(FZ_E_BADARG, f"sizes sum to {n} but {self._signer_count(vk)} keys were given")
        m = n if valid is None else int(np.count_nonzero(np.asarray(valid).reshape(n)))
        if m == 0:
            return np.zeros(0, dtype=np.int64)
        with DeviceScope() as s:
            dK = self._take(s, vk, (n, 2, self.d))
            dO = self._new(s, (n,), np.uint32)
            self.ctx.sort_by_vk_string_ragged_dev(self.P, dK.ptr, n, off, valid, dO.ptr)
            return dO.numpy()[:m].astype(np.int64)

    def hash_ag_many_dev(self, vk, messages, sizes, valid=None, scope=None):
        """Everything the many-committee calls derive from the keys and messages of G committees (sizes = signers per committee,
        concatenated as aggregate_many takes them), computed ON THE DEVICE: -> (dC [sum N][d] challenges c_hat, dAl [sum N][d]
        aggregation coefficients alpha_hat, offsets [G + 1]), both in the callers' row order.  valid ([sum N] booleans, None:
        all): hash_ag of each committee runs over its signers with valid[i] set, the others' rows of dAl are zero.  Only the
        key sort runs on the host, and with key_sort="device" not even that: the keys are then not downloaded and the digests
        stay on the device.  dC and dAl are the caller's to free, or with `scope` that DeviceScope's (as hash_ag_dev).
        Raises FusionHipError(FZ_E_UNSUPPORTED) for parameter sets the kernel does not cover, whatever self.hash_ag says."""
        if scope is None:
            with DeviceScope() as tmp:
                dC, dAl, off = self.hash_ag_many_dev(vk, messages, sizes, valid, tmp)
                return tmp.release(dC), tmp.release(dAl), off
        m = _Committees(self, scope, vk, messages, self._many_sizes(vk, messages, sizes), device_only=True)
        m.keys_dev()
        if not m.sort_dev:
            m.keys_host()
        m.challenges()
        return m.dC, m.alpha_hat(valid), m.off

    def _hash_ag_many(self, scope, vk, messages, sizes):
        """hash_ag for G independent aggregates whose signers are concatenated (aggregate g = rows off[g]:off[g+1]; sizes as
        _many_sizes passed them): ONE device pass for all challenges, then _Committees.alpha_hat: -> (the call's _Committees, with
        c_hat on the device (dC); dAl [sum N][d]), the buffers in `scope`.  Unless the sort runs on the device the challenge pass
        reads the host copy of the keys, which is made first."""
        m = _Committees(self, scope, vk, messages, sizes)
        if not m.sort_dev:
            m.keys_host(adopt=True)
        m.challenges()
        return m, m.alpha_hat()

    def aggregate_many(self, vk, messages, sig, sizes):
        """G independent aggregate() calls (fusion.py:655; the reference is called once per aggregate) as one batch:
        vk [sum N][2][d], messages (sum N of them), sig [sum N][l][d] (numpy or DeviceArray) hold the signers of aggregate 0,
        then of aggregate 1, ...; sizes = signers per aggregate (they may differ).  -> [G][l][d]; row g equals
        aggregate(params, keys_g, messages_g, signatures_g).signature_hat.  One launch for all aggregates."""
        sizes = self._many_sizes(vk, messages, sizes)
        with DeviceScope() as s:
            m, dAl = self._hash_ag_many(s, vk, messages, sizes)
            dS = self._take(s, sig, (m.n, self.l, self.d))
            dO = self._new(s, (m.g, self.l, self.d))
            self.ctx.aggregate_core_ragged_dev(dS.ptr, dAl.ptr, m.off, self.l, dO.ptr)
            return dO.numpy()

    def verify_many(self, vk, messages, aggregates, sizes):
        """G independent verify() calls (fusion.py:680-728) as one batch; aggregates [G][l][d].  -> list of (bool, reason).
        One launch for all verification targets, one for all verifications, verdicts read once."""
        sizes = [int(x) for x in sizes]
        g = len(sizes)
        out = self._one_by_one(self.verify, vk, messages, aggregates, (self.l, self.d), sizes)   # the capacity check comes first
        if out is not None:
            return out
        sizes = self._many_sizes(vk, messages, sizes)
        with DeviceScope() as s:
            m, dAl = self._hash_ag_many(s, vk, messages, sizes)
            dL, dR = m.halves_dev()
            dS = self._take(s, aggregates, (g, self.l, self.d))
            dV, dT = self._new(s, (g,)), self._targets(s, dL, dR, m.dC, dAl, m.off)
            self.ctx.verify_with_target_batch_async_dev(self._A_dev().ptr, dS.ptr, dT.ptr, g, self.l, int(self.params.beta_vf),
                                                        int(self.params.omega_vf), dV.ptr)
            return [_verdict(c) for c in dV.numpy()]

    # ---- many aggregates at once, straight from the bytes (not in the reference) ---------
    def _aggregate_groups(self, vk, messages, data, sizes, screened, encoded, verify):
        """aggregate_many_encoded, and with `verify` aggregate_verify_many_encoded: ONE body, so that each step is written once and
        the order of the steps -- what the stream sees -- can be read off it.  The records up, their status words, the check
        over all records, the challenge pass, the host copy of the keys unless the sort runs on the device, the download of the
        codes, hash_ag over the records with code 0, the fused launch, the result.  The check is the range check, or with
        `screened` the keyed verification, which reads the keys and c_hat on the device and so comes behind the challenge pass.
        Where a launch reads them there (`screened`, `verify`) the keys go to the device first and c_hat stays there; else
        nothing needs c_hat on the device, and the pass comes behind the keys' host copy."""
        nrows, bound, rb, data, n, sizes = self._signature_groups(vk, messages, data, sizes)
        g, keyed = len(sizes), screened or verify
        if g == 0:
            return self._aggregates_out(None, None, 0, encoded, np.zeros(0, dtype=np.int32)) + (([],) if verify else ())
        with DeviceScope() as s:
            m = _Committees(self, s, vk, messages, sizes)
            dB, dV = self._records_dev(s, data, n, rb), self._new(s, (n,))
            if not screened:
                self.ctx.check_records_async_dev(dB.ptr, n, nrows, bound, dV.ptr)       # beside the challenge pass
            if keyed:
                dK = m.keys_dev()
                m.challenges()
            if screened:
                self.ctx.verify_encoded_async_dev(self._A_dev().ptr, dB.ptr, n, self.l, bound, 0, dK.ptr, m.dC.ptr, dV.ptr)
            if not m.sort_dev:
                m.keys_host()
            if not keyed:
                m.challenges(keep=False)
            codes = dV.numpy()
            dAl = m.alpha_hat(codes == 0)
            dP, dO = self._new(s, (g, self.l, self.d), np.int64), self._new(s, (g, self.l, self.d))
            if not verify:
                self.ctx.aggregate_encoded_ragged_async_dev(dB.ptr, dAl.ptr, dV.ptr, m.off, self.l, bound, dP.ptr, self.l * self.d, dO.ptr)
                return self._aggregates_out(s, dO, g, encoded, codes)
            dT, dW = self._new(s, (g, self.d), np.int64), self._new(s, (g,))
            self.ctx.aggregate_target_encoded_ragged_async_dev(dB.ptr, dAl.ptr, dV.ptr, dK.ptr, m.dC.ptr, m.off, self.l, bound, dP.ptr,
                                                               self.l * self.d, dT.ptr, self.d, dO.ptr)
            self.ctx.verify_partials_batch_async_dev(self._A_dev().ptr, dP.ptr, self.l * self.d, dT.ptr, self.d, g, self.l,
                                                     int(self.params.beta_vf), int(self.params.omega_vf), dW.ptr)
            out = self._aggregates_out(s, dO, g, encoded, codes)
            accepted = np.add.reduceat((codes == 0).astype(np.int64), m.off[:-1])
            verdicts = [None if a == 0 else (False, VERDICT_REASONS[1]) if a > self.params.capacity else _verdict(c)
                        for a, c in zip(accepted, dW.numpy())]
            return out + (verdicts,)

    def aggregate_many_encoded(self, vk, messages, data, sizes, screened=False, encoded=False):
        """G independent aggregate_encoded calls (screened=True: aggregate_encoded_screened calls) as one batch: vk [sum N][2][d]
        (numpy or DeviceArray), messages and `data` (sum N "signature" records in every form decode takes) hold the signers of
        aggregate 0, then of aggregate 1, ...; sizes = signers per aggregate (they may differ, each at least 1).
        -> (aggregates [G][l][d] int32, codes int32 [sum N]): codes[i] is 0 or 6 (ENCODING_REASONS), with screened=True 0, 3
        (SIGNATURE_REASONS) or 6; row g is bit for bit what the single call returns for group g alone, and all zero where that
        call returns None (no accepted signer: hash_ag does not run for the group).
        encoded=True: bytes in, bytes out -- the aggregates are never downloaded as rows: -> (records uint8
        [G][encoded_size(params, "aggregate")], codes, aggregate_codes int32 [G]), aggregate_codes[g] 0 or 4 as encode gives it.
        One upload of the bytes, one range check (or one keyed verification) over all records whose status words stay on the
        device as the skip words, one challenge pass, hash_ag per group over its accepted signers on the thread pool of
        aggregate_many, one upload + transform of all coefficients, ONE launch for all groups (fz_aggregate_encoded_ragged_async),
        one download.  Sizes that do not sum to the numbers of records, keys and messages, a size below 1, or a length that is
        not whole records raise FusionHipError(FZ_E_BADARG) before the device is touched; no records and sizes == [] return
        empty arrays without a device."""
        return self._aggregate_groups(vk, messages, data, sizes, screened, encoded, False)

    def _signature_groups(self, vk, messages, data, sizes):
        """the input of the calls that take groups of "signature" records, refused with FusionHipError(FZ_E_BADARG) unless it is
        whole records and the sizes, each at least 1, sum to the numbers of records, keys and messages; no device is touched:
        -> (nrows, bound, rb, data, n, sizes)"""
        nrows, _, bound, _, rb = _encoding(self.params, "signature")
        data, n = _records_input("signature", data, rb)
        sizes = self._many_sizes(vk, messages, sizes)
        self._check_dev(vk, (sum(sizes), 2, self.d))
        if sum(sizes) != n:
            raise FusionHipError(FZ_E_BADARG, f"sizes sum to {sum(sizes)} but {n} records were given")
        return nrows, bound, rb, data, n, sizes

    def _aggregates_out(self, s, dO, g, encoded, codes):
        """how the many-committee calls from the bytes hand back the g aggregates dO [g][l][d] holds on the device, in front of
        the records' `codes`: -> (rows [g][l][d] int32, codes), or with encoded (records uint8 [g][encoded_size(params,
        "aggregate")], codes, aggregate_codes int32 [g]) -- the aggregates are then never downloaded as rows; g == 0: the empty
        arrays, no device"""
        _, _, abound, _, arb = _encoding(self.params, "aggregate")
        if g == 0:
            return (np.zeros((0, arb), dtype=np.uint8), codes, np.zeros(0, dtype=np.int32)) if encoded else \
                (np.zeros((0, self.l, self.d), dtype=np.int32), codes)
        if not encoded:
            return dO.numpy(), codes
        dR, dW = self._new(s, (g, arb), np.uint8), self._new(s, (g,))
        self.ctx.encode_records_async_dev(dO.ptr, g, self.l, True, abound, dR.ptr, dW.ptr)
        return dR.numpy(), codes, dW.numpy()

    # ---- aggregate and verify in one pass, straight from the bytes (not in the reference) ---------
    def aggregate_verify_many_encoded(self, vk, messages, data, sizes, encoded=False):
        """aggregate_many_encoded followed, per group, by verify() of the group's aggregate on its accepted signers, as an
        aggregator that checks its own output does, in ONE pass: -> (aggregates [G][l][d] int32, codes int32 [sum N], verdicts),
        or with encoded=True (records uint8 [G][encoded_size(params, "aggregate")], codes, aggregate_codes int32 [G], verdicts).
        Rows, codes (0 or 6) and aggregate_codes are bit for bit aggregate_many_encoded's; verdicts[g] is bit for bit
        verify(vk_g[ok], messages_g[ok], aggregate_g) over the group's records with code 0 -- (bool, reason), the capacity
        refusal for more than params.capacity accepted signers included (no arithmetic decides it, and the aggregate is still
        returned) -- and None where the group has no accepted signer (its row is zero).
        One upload of the bytes, one range check whose status words stay on the device as the skip words, one upload of vk (the
        challenge pass and the fused launch read the same copy), one challenge pass with c_hat kept on the device, hash_ag ONCE
        per group -- the two calls in sequence run it, the key sort and the challenge pass twice --, one upload + transform of
        the coefficients, ONE launch for all aggregates' and all targets' int64 sums
        (fz_aggregate_target_encoded_ragged_async), one for all verdicts straight from the sums
        (fz_verify_partials_batch_async), one download.  Refusals are aggregate_many_encoded's, raised before the device is
        touched; no records and sizes == [] return empty arrays and [] without a device."""
        return self._aggregate_groups(vk, messages, data, sizes, False, encoded, True)

    def aggregate_verify_encoded(self, vk, messages, data):
        """aggregate_encoded followed by verify() of the result on the accepted signers, in one pass (the many-committee form
        with one group): -> (aggregate [l][d] int32, codes int32 [N], (ok, reason)).  aggregate and codes are
        aggregate_encoded's; the verdict is bit for bit verify(vk[ok], messages[ok], aggregate) over the records with code 0,
        its capacity refusal included.  No canonical record (or N == 0): (None, codes, None).  hash_ag, the challenge pass and
        the key sort run once where aggregate_encoded + verify run them twice.  A length that is not N whole records, or
        numbers of keys / messages other than N, raise FusionHipError(FZ_E_BADARG) before the device is touched."""
        n = _records_input("signature", data, _encoding(self.params, "signature")[4])[1]
        aggs, codes, verdicts = self.aggregate_verify_many_encoded(vk, messages, data, [n] if n else [])
        if not verdicts or verdicts[0] is None:
            return None, codes, None
        return aggs[0], codes, verdicts[0]

    def verify_many_encoded(self, vk, messages, data, sizes):
        """G independent verify_encoded calls as one batch: `data` holds G "aggregate" records (every form decode takes), vk and
        messages the signers of aggregate 0, then of aggregate 1, ...; sizes = signers per aggregate.  -> [(bool, reason)] * G,
        entry g equal to verify_encoded of group g alone: a record that is not canonical gives (False, ENCODING_REASONS[6]).
        One hash_ag pass for all groups, one launch for all verification targets, one for all verifications straight from the
        bytes, verdicts read once; the aggregates' int32 rows never exist on the device.  Sizes that do not sum to the numbers
        of keys and messages, a size below 1, or anything but len(sizes) whole records raise FusionHipError(FZ_E_BADARG) before
        the device is touched."""
        _, _, bound, _, rb = _encoding(self.params, "aggregate")
        data, nrec = _records_input("aggregate", data, rb)
        sizes = self._many_sizes(vk, messages, sizes)
        self._check_dev(vk, (sum(sizes), 2, self.d))
        g = len(sizes)
        if nrec != g:
            raise FusionHipError(FZ_E_BADARG, f"{nrec} 'aggregate' records but {g} sizes")
        if g == 0:
            return []
        out = self._one_by_one(self.verify_encoded, vk, messages, data, (rb,), sizes)      # the capacity check first, as in verify_many
        if out is not None:
            return out
        with DeviceScope() as s:
            m, dAl = self._hash_ag_many(s, vk, messages, sizes)
            dL, dR = m.halves_dev()
            dB = self._records_dev(s, data, g, rb)
            dV, dT = self._new(s, (g,)), self._targets(s, dL, dR, m.dC, dAl, m.off)
            self.ctx.verify_encoded_async_dev(self._A_dev().ptr, dB.ptr, g, self.l, bound, dT.ptr, 0, 0, dV.ptr)
            return [_verdict(c) for c in dV.numpy()]


def _offsets(sizes):
    """committee sizes -> the int64 offsets [G + 1] of the committees' first rows, and the end"""
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _order_of_valid(order, off, valid):
    """a host order of all rows, committee after committee (offsets `off`), filtered by valid [N] (None: all): -> (the valid rows
    in that order, the offsets of the committees that keep a row).  The sort is stable, so this is the order of the valid rows
    sorted alone, as in screened_alpha_coefficients."""
    if valid is None:
        return order, off
    keep = np.asarray(valid, dtype=bool).reshape(len(order))[order]
    counts = np.add.reduceat(keep.astype(np.int64), off[:-1]) if len(order) else np.zeros(0, dtype=np.int64)
    return order[keep], _offsets(counts[counts > 0])


class _Committees:
    """The inputs of ONE many-committee call of BatchScheme `bs`: the keys `vk` [sum N][2][d] (numpy or DeviceArray) and messages of
    G committees of `sizes` signers each, concatenated.  Built once per call, inside the call's DeviceScope, touching no device.
    It owns
      off, n, g   the offsets [G + 1], made once; sum N; G
      form        "host" or "device": where hash_ag runs, decided HERE, once, by bs._hash_ag_form (device_only: the device form
                  whatever that says, and no fall-back from it -- hash_ag_many_dev's contract)
      sort_dev    does the device form sort the keys on the device?  THE predicate for "no host copy of the keys is needed":
                  then the digests stay on the device as well
      vk, keys    the keys as they came, and what the challenge pass and an upload of the keys read: vk, its host copy where
                  keys_host(adopt=True) made it, dK once that exists
    and what the call derives, each made at most once by the method that says where it lives (the attributes are None before):
      keys        keys_dev() -> dK [N][2][d] on the device; keys_host() -> (L, R) [N][d] on the host; halves_dev() -> the halves
                  on the device, uploads of L and R or -- sort_dev -- dK taken apart there
      challenges  challenges() runs the pass and leaves c_hat on the device (dC), on the host (c_hat) or both, and the digests
                  on the host (pre) or -- sort_dev -- on the device (dP [N][32]), as the form needs them
      the rest    host_copies() -> (c_hat, L, R, pre), downloads of what is on the device only; alpha_hat() uploads the digests
                  where hash_ag's device form finds them on the host
    alpha_hat() is the one place that chooses between the forms of hash_ag.  Nothing here moves a transfer: a method called a
    second time returns what the first call made, and the CALLER's order of first calls is the order the stream sees.  Device
    buffers are the scope's (or the caller's own DeviceArray), never this object's."""

    def __init__(self, bs, scope, vk, messages, sizes, device_only=False):
        self.bs, self.scope, self.vk, self.keys, self.messages, self.device_only = bs, scope, vk, vk, messages, device_only
        self.off = _offsets(sizes)
        self.n, self.g = int(self.off[-1]), len(sizes)
        form = bs._hash_ag_form(sizes)                      # every call asks once, here; device_only overrules the answer
        self.form = "device" if device_only else form
        self.sort_dev = self.form == "device" and bs.key_sort == "device"
        self.dK = self.dC = self.dP = self.L = self.R = self.c_hat = self.pre = None

    def keys_dev(self):
        if self.dK is None:
            self.dK = self.keys = self.bs._take(self.scope, self.keys, (self.n, 2, self.bs.d))
        return self.dK

    def keys_host(self, adopt=False):
        """(L, R); adopt: the challenge pass and keys_dev() read this copy from here on (an upload, where vk came as a DeviceArray).
        sort_dev, so only after the device form refused: the copy of the keys that form read is the one downloaded"""
        if self.L is None:
            vk, self.L, self.R = self.bs._split_vk(self.dK if self.sort_dev else self.vk)
            if adopt:
                self.keys = vk
        return self.L, self.R

    def halves_dev(self):
        bs, s = self.bs, self.scope
        if not self.sort_dev:
            return tuple(bs._up(s, half) for half in self.keys_host())
        dL, dR = bs._new(s, (self.n, bs.d)), bs._new(s, (self.n, bs.d))
        bs.ctx.vk_halves_dev(self.keys_dev().ptr, self.n, dL.ptr, dR.ptr)
        return dL, dR

    def host_copies(self):
        """-> (c_hat, L, R, pre) on the host: each a download of the device's copy unless it is there"""
        if self.c_hat is None:
            self.c_hat = self.dC.numpy()
        L, R = self.keys_host()
        if self.pre is None:
            self.pre = self.dP.numpy()
        return self.c_hat, L, R, self.pre

    def challenges(self, keep=True):
        """the challenge pass in the way of the form.  Host form: c_hat and the digests on the host, and c_hat on the device unless
        keep is False (hash_ag reads the host copy; nothing then needs it there).  Device form: from dK, c_hat stays on the device
        and the digests come back -- or, sort_dev, stay there as well (fz_challenge_hat_msgs_keep_dev: nothing is downloaded and
        nothing waited for).  A parameter set the device pipeline does not cover takes the host pipeline as everywhere
        (BatchScheme._challenges_both), which leaves host copies in every form."""
        bs, s = self.bs, self.scope
        if self.form == "device":
            dK = self.keys_dev()
            if self.sort_dev and bs.device_hash:
                blob, moff = hostpipe._pack_messages(self.messages)
                dC, dP = bs._new(s, (self.n, bs.d)), bs._new(s, (self.n, 32), np.uint8)
                try:
                    bs.ctx.challenge_msgs_keep_dev(bs.P, dK.ptr, blob, moff, self.n, dC.ptr, dP.ptr)
                    self.dC, self.dP = dC, dP
                    return
                except FusionHipError as e:
                    if e.code != FZ_E_UNSUPPORTED:
                        raise
                    bs.device_hash = False
            self.dC, self.c_hat, self.pre = bs._challenges_both(dK, self.messages, want_host=False, scope=s, want_pre=True)
        else:
            with DeviceScope() as t:                        # keep=False: c_hat leaves the device once its host copy is here
                dC, self.c_hat, self.pre = bs._challenges_both(self.keys, self.messages, scope=s if keep else t)
            self.dC = dC if keep else None

    def alpha_hat(self, valid=None):
        """hash_ag's coefficients for the G committees, over the signers with valid[i] set (None: all): -> dAl [sum N][d] in the
        scope, zero rows for the others.  THE place where the many-committee calls branch on the form.
        Device form: a wave per committee, from dK and dC where they are -- c_hat is not downloaded and no coefficient uploaded --,
        the keys sorted by str(vk) on the host (one C call over all committees; fz_hash_ag_ragged_dev takes the order) or, sort_dev,
        on the device as well (fz_hash_ag_ragged_sorted_dev), the digests uploaded unless they are there.  FZ_E_UNSUPPORTED, for a
        parameter set the kernel does not cover, turns the device form off for the BatchScheme, which stays there, and this call
        goes on with the host form on host_copies().
        Host form: one host thread per committee for its sort + serial SHAKE-256 (the sponges are what bounds a lone aggregate:
        independent aggregates hide each other's), zero rows without hashing for a committee with no valid signer, then ONE
        upload + transform of all rows."""
        bs, off, g, n = self.bs, self.off, self.g, self.n
        if self.form == "device":
            try:
                if self.sort_dev:
                    entry, rows = bs.ctx.hash_ag_ragged_sorted_dev, (off, valid)
                else:
                    order = hostpipe.sort_by_vk_string_ragged(bs.P, *self.keys_host(), off, bs.threads)
                    entry, rows = bs.ctx.hash_ag_ragged_dev, _order_of_valid(order, off, valid)
                if self.dP is None:
                    self.dP = bs._up(self.scope, np.ascontiguousarray(self.pre, dtype=np.uint8).reshape(n, 32))
                dAl = bs._new(self.scope, (n, bs.d))
                entry(bs.P, self.dK.ptr, self.dP.ptr, self.dC.ptr, n, *rows, dAl.ptr)
                return dAl
            except FusionHipError as e:
                if e.code != FZ_E_UNSUPPORTED or self.device_only:
                    raise
                bs.device_hash_ag = False
        from concurrent.futures import ThreadPoolExecutor
        c_hat, L, R, pre = self.host_copies()
        per = max(1, bs.threads // max(1, g))

        def one(k):
            a, b = off[k], off[k + 1]
            ok = None if valid is None else valid[a:b]
            if ok is not None and not ok.any():
                return np.zeros((b - a, bs.d), dtype=np.int32)
            return screened_alpha_coefficients(bs.P, L[a:b], R[a:b], pre[a:b], c_hat[a:b], ok, per)[1]
        with ThreadPoolExecutor(max_workers=min(g, bs.threads)) as pool:      # the C calls release the GIL
            alpha = np.concatenate(list(pool.map(one, range(g))))
        return bs._alpha_hat(self.scope, alpha)


def _verdict(code):
    """a verification's code -> (ok, reason): the reference's reason strings, and for a record that is not canonical (6, from
    the bytes only) the encoding's"""
    code = int(code)
    return code == 0, (ENCODING_REASONS[6] if code == 6 else VERDICT_REASONS[code])


def _integer_seeds(seeds):
    """the seeds as they came when they are a flat sequence of integers (Python or numpy ones, of any sign and size; no
    booleans), else FusionHipError(FZ_E_BADARG): a float would be truncated and a nested list fail half way otherwise"""
    if isinstance(seeds, np.ndarray):
        if seeds.ndim == 1 and (seeds.dtype.kind in "iu" or seeds.size == 0):
            return seeds
        raise FusionHipError(FZ_E_BADARG,
                             f"seeds of shape {seeds.shape} and type {seeds.dtype}: a flat sequence of integers expected")
    try:
        seeds = list(seeds)
    except TypeError:
        raise FusionHipError(FZ_E_BADARG,
                             f"seeds of type {type(seeds).__name__}: a flat sequence of integers expected") from None
    for i, v in enumerate(seeds):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise FusionHipError(FZ_E_BADARG, f"seed {i} is a {type(v).__name__}: a flat sequence of integers expected")
    return seeds


def _seed_array(seeds):
    """the seeds as a uint64 array when every one is a non-negative integer below 2^64 - 1 (what the C and device samplers
    take), else None.  One numpy conversion instead of a Python loop: 0.25 us per seed was most of what a 1024-key
    keygen_batch spent on the host."""
    try:
        a = np.asarray(seeds)
    except (OverflowError, ValueError, TypeError):
        a = None
    if a is not None and a.ndim == 1 and a.dtype.kind == "u":
        a = a.astype(np.uint64, copy=False)
        return a if a.size == 0 or int(a.max()) < 2 ** 64 - 1 else None
    if a is not None and a.ndim == 1 and a.dtype.kind == "i":
        return a.astype(np.uint64) if a.size == 0 or int(a.min()) >= 0 else None
    # objects, floats (numpy's choice for lists that mix negative and huge ints), nested input: element by element
    vals = [int(s) for s in seeds]
    if any(v < 0 or v >= 2 ** 64 - 1 for v in vals):
        return None
    return np.array(vals, dtype=np.uint64)


# ---- conversions between the array face and the drop-in object face ----------------------------------------
def _own(rows):
    """a private int32 copy: the objects keep their rows as they are until somebody reads their lists
    (algebra/polynomials.py, storage note), so they must not alias an array the caller may write to afterwards"""
    return np.array(rows, dtype=np.int32, copy=True)


def vk_to_object(params, vk_row):
    """vk [2][d] -> fusion.fusion.OneTimeVerificationKey"""
    import fusion.fusion as F
    vk_row = _own(vk_row)
    return F.OneTimeVerificationKey(left_vk_hat=F._column(params, vk_row[0:1]), right_vk_hat=F._column(params, vk_row[1:2]))


def sk_to_object(params, seed, sk_rows):
    """sk_hat [2][l][d] -> fusion.fusion.OneTimeSigningKey"""
    import fusion.fusion as F
    sk_rows = _own(sk_rows)
    return F.OneTimeSigningKey(seed=seed, left_sk_hat=F._column(params, sk_rows[0]), right_sk_hat=F._column(params, sk_rows[1]))


def signature_to_object(params, sig_rows):
    import fusion.fusion as F
    return F.Signature(signature_hat=F._column(params, _own(sig_rows)))


def signature_from_object(params, sig):
    import fusion.fusion as F
    return F._rows_of(sig.signature_hat, params.modulus)


def vk_from_object(params, vk):
    import fusion.fusion as F
    return np.concatenate([F._rows_of(vk.left_vk_hat, params.modulus), F._rows_of(vk.right_vk_hat, params.modulus)])
