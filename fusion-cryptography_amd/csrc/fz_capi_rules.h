// fz_capi_rules.h -- the rules the host units of the older half of the C ABI share (fz_capi.hip, fz_staged_capi.hip), written once.
// Host code only; everything is private to the unit that includes it.
#ifndef FZ_CAPI_RULES_H
#define FZ_CAPI_RULES_H

#include "fz_internal.h"
#include "../../include/fusion_hip.h"

static int needs_transforms(const fz_ctx *ctx) {
    return ctx->logd >= 0 ? FZ_OK : fz_set_error(FZ_E_UNSUPPORTED, "ring-only context (created with root 0) has no transforms");
}
// how an entry begins unless its own order says otherwise: its arguments (the context first), then the context's device made current
#define FZ_ENTER(ctx, args_ok, ...) do { FZ_REQUIRE((ctx) && (args_ok), __VA_ARGS__); FZ_DEV(ctx); } while (0)

#endif
