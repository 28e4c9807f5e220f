// fz_transforms.hip -- three kernel families compiled as ONE unit, in this order: apart, the compiler schedules the radix-4 inverse's
// users (ntt_inv4, ntt_jobs4, polymul_fused) differently from the one-file original (profiles/r09_split_isa.txt).
#include "fz_ntt.hip"
#include "fz_scheme_fused.hip"
#include "fz_polymul.hip"
