// Host-only driver of avcer_amd/csrc/gemm_forms.h for tests/test_gemm_forms_cpu.py.  Prints the dtype table, then for every
// shape line on stdin (the columns of tests/golden/gemm_forms.csv up to short_in) what choose_gemm picks, the tile its launcher
// would take, and why each of the two special forms cannot take the shape ("-": it can).  Decides nothing itself.
#include <cstdio>
#include <cstring>

#include "gemm_forms.h"

int main() {
    for (int i = 0; i < kGemmForms; ++i) {
        const GemmForm& f = kGemmForm[i];
        printf("row %d %d %d %d %d %d inverse %d bytes %d %d bk %d a_split %d ovec %d family %d\n", i, f.a_kind, f.o_kind, f.w_copy, f.form, f.mode,
               gemm_dtype(f.a_kind, f.o_kind, f.w_copy >= W_SPLIT, f.form), gemm_in_bytes(i), gemm_out_bytes(i), gemm_bk(i), (int)gemm_a_split(i),
               gemm_ovec(i), gemm_family(i));
    }
    printf("inverse_none %d %d\n", gemm_dtype(KIND_SP32, KIND_BF16, true, FORM_STAGED), gemm_dtype(KIND_F32, KIND_F32, false, FORM_SKINNY));
    printf("splits %d %d %d %d\n", (int)gemm_weight_splits(2, 64, 32), (int)gemm_weight_splits(4, 64, 32), (int)gemm_weight_splits(2, 32, 32),
           (int)gemm_weight_splits(2, 64, 48));
    long M;
    int N, cin, kh, kw, pad, groups, x2_cin, tile_n, tile_m, slots, a_kind, o_kind, x3, copies, short_in;
    while (scanf("%ld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &M, &N, &cin, &kh, &kw, &pad, &groups, &x2_cin, &tile_n, &tile_m, &slots, &a_kind,
                 &o_kind, &x3, &copies, &short_in) == 16) {
        // M positions as a batch of 1 x 1 outputs under a kh x kw window; short_in: the input ends one row above the last tap
        avcer_conv_desc d;
        memset(&d, 0, sizeof d);
        d.batch = (int)M; d.out_h = d.out_w = 1; d.in_h = kh - 2 * pad - short_in; d.in_w = kw - 2 * pad;
        d.cin = cin; d.kh = kh; d.kw = kw; d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1; d.pad_h = d.pad_w = pad;
        d.n = N; d.groups = groups; d.x2_cin = x2_cin; d.x2_stride = 1; d.tile_n = tile_n; d.tile_m = tile_m;
        const bool x2 = x2_cin > 0, fast = gemm_fast_gather(d, 32);
        const long K = (long)kh * kw * cin + x2_cin;
        const char* no_direct = direct_cannot(d, K, x2, fast);
        const char* no_skinny = skinny_cannot(d, K, x2, fast);
        const int dtype = choose_gemm(a_kind, o_kind, x3 != 0, (unsigned)copies, d, x2, slots);  // resets d's hints for the skinny form
        int tile = 0;
        if (dtype >= 0) {
            const int form = kGemmForm[dtype].form;
            tile = form == FORM_SKINNY ? skinny_tile_m(M, N, gemm_groups(d), slots, d.tile_m) : form == FORM_DIRECT ? direct_tile_m(M, N, slots, d.tile_m)
                                                                                                               : staged_tile_n(M, N, K, slots, d.tile_n);
        }
        printf("choice %d %d|%s|%s\n", dtype, tile, no_direct ? no_direct : "-", no_skinny ? no_skinny : "-");
    }
    return 0;
}
