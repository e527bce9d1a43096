// window.hip -- what the bit window of the command loop (brx_hot.S, TAKE / REFILL_CORE) costs per take on gfx950: the 64-bit
// shifted window (rounds 2 - 6) against the fixed dword pair + v_alignbit_b32 view (round 7), on one lone wave and on
// 16 waves per CU (4096 waves, 10 KiB of LDS each as in the decoder, so that a CU holds exactly 16).
//   chains : 64 dependent v_lshrrev_b64 / v_alignbit_b32 / v_lshrrev_b32 / other VOP3 instructions of the loop
//   takes  : 64 takes of 6 bits, each followed by the lookup's first reader (v_bfrev_b32 of the view); the refill is out of
//            line behind the loop and is taken by the real carry / borrow: one take in 5.33, alice29's rate.
// Build: hipcc --offload-arch=gfx950 -O2 window.hip -o window        Run: ./window  (prints ticks of s_memtime per take)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef unsigned long long u64;
typedef unsigned int u32;
#define ITERS 200
// 64 distinct two-digit ids: the take's stub and return labels (numeric local labels 7xx / 8xx)
#define R8(M, a) M(a##0) M(a##1) M(a##2) M(a##3) M(a##4) M(a##5) M(a##6) M(a##7)
#define R64(M) R8(M, 0) R8(M, 1) R8(M, 2) R8(M, 3) R8(M, 4) R8(M, 5) R8(M, 6) R8(M, 7)
// registers: v[10:11] window / v10 view, v[12:13] refill pair or the dword pair, v14 staged input, v15 the reader's result;
// s90 SNAV or C, s91 take width, s92 WL, s93 WLSTOP (never reached), s94 T0, s95 loop counter
#define OLD_TAKE(id) "v_lshrrev_b64 v[10:11], s91, v[10:11]\n s_sub_u32 s90, s90, s91\n s_cbranch_scc1 7" #id "f\n 8" #id ":\n v_bfrev_b32 v15, v10\n"
#define OLD_STUB(id) "7" #id ":\n v_readlane_b32 s94, v14, s92\n v_mov_b32 v13, 0\n s_nop 1\n v_mov_b32 v12, s94\n s_add_u32 s90, s90, 32\n" \
                     "v_lshlrev_b64 v[12:13], s90, v[12:13]\n v_or_b32 v10, v10, v12\n v_or_b32 v11, v11, v13\n s_add_u32 s92, s92, 1\n" \
                     "s_cmp_lg_u32 s92, s93\n s_cbranch_scc1 8" #id "b\n"
#define NEW_TAKE(id) "s_add_u32 s90, s90, s91\n s_cbranch_scc1 7" #id "f\n 8" #id ":\n v_alignbit_b32 v10, v13, v12, s90\n v_bfrev_b32 v15, v10\n"
#define NEW_STUB(id) "7" #id ":\n v_readlane_b32 s94, v14, s92\n v_mov_b32 v12, v13\n s_sub_u32 s90, s90, 32\n s_add_u32 s92, s92, 1\n" \
                     "v_mov_b32 v13, s94\n s_cmp_lg_u32 s92, s93\n s_cbranch_scc1 8" #id "b\n"
// second arm: the next dword waits in v11, fetched at the previous refill (one instruction more, no readlane -> VALU hand-over)
#define PRE_STUB(id) "7" #id ":\n v_mov_b32 v12, v13\n v_mov_b32 v13, v11\n s_add_u32 s92, s92, 1\n v_readlane_b32 s94, v14, s92\n s_sub_u32 s90, s90, 32\n" \
                     "s_cmp_lg_u32 s92, s93\n v_mov_b32 v11, s94\n s_cbranch_scc1 8" #id "b\n"
#define CH_B64(id) "v_lshrrev_b64 v[10:11], 1, v[10:11]\n"
#define CH_ALIGN(id) "v_alignbit_b32 v10, v13, v10, s91\n"
#define CH_B32(id) "v_lshrrev_b32 v10, 1, v10\n"
#define CH_ALIGN_K(id) "v_alignbit_b32 v10, v10, v10, 1\n"      // one VGPR, constant shift: is it the three register reads?
#define CH_LSHL_ADD(id) "v_lshl_add_u32 v10, v10, 1, v13\n"     // another three-operand VOP3 (the lookups' address arithmetic)
#define CH_BFE(id) "v_bfe_u32 v10, v10, 0, s91\n"               // TAKE_EXTRA's field extract
#define NONE(id)

#define TIMED(NAME, INIT, BODY, STUBS)                                                                                   \
    __global__ void NAME(u64 *out) {                                                                                     \
        __shared__ u32 lds[2560]; /* 10 KiB: 16 waves per CU */                                                          \
        lds[threadIdx.x] = threadIdx.x;                                                                                  \
        __syncthreads();                                                                                                 \
        u64 t0, t1;                                                                                                      \
        u32 v = lds[threadIdx.x ^ 1] * 0x9e3779b1u;                                                                      \
        asm volatile("v_mov_b32 v10, %2\n v_mov_b32 v11, %2\n v_mov_b32 v12, %2\n v_mov_b32 v13, %2\n v_mov_b32 v14, %2\n"   \
                     "s_mov_b32 s91, 6\n s_mov_b32 s92, 0\n s_mov_b32 s93, 0x7fffffff\n s_mov_b32 s95, %3\n" INIT "\n"    \
                     "s_memtime %0\n s_waitcnt lgkmcnt(0)\n"                                                              \
                     "1:\n" BODY "s_sub_u32 s95, s95, 1\n s_cbranch_scc0 1b\n"                                           \
                     "s_memtime %1\n s_waitcnt lgkmcnt(0)\n s_branch 2f\n" STUBS "2:\n"                                   \
                     : "=s"(t0), "=s"(t1) : "v"(v), "n"(ITERS - 1)                                                        \
                     : "vcc", "scc", "memory", "s90", "s91", "s92", "s93", "s94", "s95", "v10", "v11", "v12", "v13", "v14", "v15"); \
        if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;                                                                  \
    }
TIMED(k_ch_b64, "", R64(CH_B64), R64(NONE))
TIMED(k_ch_align, "", R64(CH_ALIGN), R64(NONE))
TIMED(k_ch_b32, "", R64(CH_B32), R64(NONE))
TIMED(k_ch_align_k, "", R64(CH_ALIGN_K), R64(NONE))
TIMED(k_ch_lshl_add, "", R64(CH_LSHL_ADD), R64(NONE))
TIMED(k_ch_bfe, "", R64(CH_BFE), R64(NONE))
TIMED(k_old, "s_mov_b32 s90, 0", R64(OLD_TAKE), R64(OLD_STUB))
TIMED(k_new, "s_mov_b32 s90, -32", R64(NEW_TAKE), R64(NEW_STUB))
TIMED(k_pre, "s_mov_b32 s90, -32", R64(NEW_TAKE), R64(PRE_STUB))

int main() {
    const int full = 4096;
    u64 *o;
    if (hipMalloc(&o, full * sizeof(u64)) != hipSuccess) { printf("no device\n"); return 1; }
    std::vector<u64> h(full);
#define RUN(K, WHAT) { double r[2][2]; int w = 0; for (int waves : {1, full}) { double best = 1e30, worst = 0; for (int rep = 0; rep < 3; rep++) { \
        hipLaunchKernelGGL(K, dim3(waves), dim3(64), 0, 0, o); if (hipMemcpy(h.data(), o, waves * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); return 1; } \
        double sum = 0; for (int i = 0; i < waves; i++) sum += (double)h[i]; const double mean = sum / waves / (64.0 * ITERS); \
        if (mean < best) best = mean; if (mean > worst) worst = mean; } r[w][0] = best; r[w][1] = worst; w++; } \
      printf("%-58s lone wave %6.2f (%6.2f)   16 waves per CU %7.2f (%7.2f)\n", WHAT, r[0][0], r[0][1], r[1][0], r[1][1]); }
    printf("ticks per take / per chain link: best of 3 launches (worst), mean over the launch's waves\n");
    RUN(k_ch_b64, "chain: v_lshrrev_b64");
    RUN(k_ch_align, "chain: v_alignbit_b32 (one SGPR operand)");
    RUN(k_ch_b32, "chain: v_lshrrev_b32");
    RUN(k_ch_align_k, "chain: v_alignbit_b32, one VGPR, constant shift");
    RUN(k_ch_lshl_add, "chain: v_lshl_add_u32");
    RUN(k_ch_bfe, "chain: v_bfe_u32 (width in an SGPR)");
    RUN(k_old, "take + refill, 64-bit shifted window (rounds 2 - 6)");
    RUN(k_new, "take + refill, fixed dword pair + v_alignbit_b32");
    RUN(k_pre, "  ... second arm: next dword prefetched into a VGPR");
    return 0;
}
