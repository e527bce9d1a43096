// runentry.hip -- what the entry of a literal run costs in the resident loops of the command loop (brx_hot.S, LIT_CTX_ENTRY) on
// gfx950: a landing of PFREE pending lanes, the context of the run's first literal, the run's bookkeeping (LIT_RUN_FAST) and
// the first literal (LIT_R_BODY_MX: tree pair through the VGPR index mode, LOOKUP2X, the entry's hand-over), on one lone wave
// and on 16 waves per CU (4096 waves, 10 KiB of LDS each as in the decoder, so that a CU holds exactly 16).
//   old : the last two pending bytes and their context info through v_readlane (VPEND, VITAB), the fields on the scalar side
//         (rounds 4 - 7: 15 scalar instructions and 4 v_readlane in front of the first literal)
//   new : every pending lane reads the info of its byte from the table in LDS inside the landing's EXEC window, splits it on the
//         vector side, one DPP shift by a lane joins the neighbours; two v_readlane at lane PFREE - 1 (round 8)
// Both arms are the instruction sequences of the loop, register for register; the data is constant (an all-zero window, table and
// context map), which no instruction's timing depends on.  Every LDS address is inside the block's 10 KiB.
// Build: hipcc --offload-arch=gfx950 -O2 runentry.hip -o runentry     Run: ./runentry  (prints ticks of s_memtime per entry)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef unsigned long long u64;
typedef unsigned int u32;
#define ITERS 200
#define R8(M, a) M(a##0) M(a##1) M(a##2) M(a##3) M(a##4) M(a##5) M(a##6) M(a##7)
#define R16(M) R8(M, 0) R8(M, 1) /* 16 entries per trip: 5 KiB of code, inside the instruction cache as the loop is */
// registers as in brx_hot.S: s8 PFREE, s9 PBASE, s52 POS, s53 SKEW, s55 FLUSHAT, s65 LBLEN, s68 RUN, s92 INS, s70 SWC, s71 MA2,
// s28 BFEB, s22 BFEBI, s3 MB, s84 .. s91 T0 .. T7, s96 CLEN; v1 lane, v6 VSH, v7 VS, v8 VPA, v12 VPEND, v18 .. v22 VT0 .. VT4,
// v23 VITAB, v28 VE, v32 the window's view, v35 VI, v36 / v37 the dword pair, v24 VR, v70 / v71 tree 0, v103 VCMAP; s95 counts
#define LAND_HEAD "s_add_u32 s90, s9, s53\n s_bfm_b64 exec, s8, 0\n v_add_u32 v19, s90, v1\n v_and_b32 v19, 0x7ff, v19\n" \
                  "s_waitcnt vmcnt(0) lgkmcnt(0)\n ds_write_b8 v19, v12\n"
#define LAND_TAIL "s_mov_b64 exec, 0x1ffff\n s_mov_b32 s8, 0\n"
#define OLD_ENTRY "s_cmp_eq_u32 s8, 0\n s_cbranch_scc1 2f\n s_sub_u32 s88, s8, 1\n s_sub_u32 s89, s8, 2\n" LAND_HEAD LAND_TAIL \
                  "v_readlane_b32 s90, v12, s88\n v_readlane_b32 s91, v12, s89\n s_add_u32 s84, s52, s53\n v_bfe_u32 v8, s84, 0, 11\n" \
                  "s_lshr_b32 s84, s90, 2\n s_lshr_b32 s85, s91, 2\n v_readlane_b32 s84, v23, s84\n v_readlane_b32 s85, v23, s85\n" \
                  "s_lshl_b32 s90, s90, 3\n s_lshl_b32 s91, s91, 3\n s_lshr_b32 s90, s84, s90\n s_lshr_b32 s91, s85, s91\n" \
                  "s_bfe_u32 s85, s90, 0x60002\n s_and_b32 s85, s85, s71\n s_bfe_u32 s89, s90, s22\n s_bfe_u32 s91, s91, s22\n" \
                  "s_or_b32 s88, s85, s91\n"
#define NEW_ENTRY "s_cmp_eq_u32 s8, 0\n s_cbranch_scc1 2f\n" LAND_HEAD \
                  "ds_read_u8 v18, v12 offset:8960\n s_waitcnt lgkmcnt(0)\n v_and_b32 v21, s3, v18\n v_lshrrev_b32 v20, 2, v18\n" \
                  "s_sub_u32 s88, s8, 1\n s_add_u32 s84, s52, s53\n v_or_b32_dpp v20, v21, v20 wave_shr:1 row_mask:0xf bank_mask:0xf\n" LAND_TAIL \
                  "v_bfe_u32 v8, s84, 0, 11\n v_readlane_b32 s89, v21, s88\n v_readlane_b32 s88, v20, s88\n"
#define RUN_FAST "s_sub_u32 s90, s55, s52\n s_cbranch_scc1 2f\n s_min_u32 s90, s90, s65\n s_cmp_gt_u32 s92, s90\n s_cbranch_scc1 2f\n" \
                 "s_sub_u32 s65, s65, s92\n s_add_u32 s52, s52, s92\n s_sub_u32 s68, s92, 1\n s_mov_b32 s92, 0\n"
#define FIRST_LIT "v_readlane_b32 s90, v103, s88\n v_bfrev_b32 v24, v32\n v_lshrrev_b32 v35, v6, v24\n s_set_gpr_idx_on s90, gpr_idx(SRC1,SRC2)\n" \
                  "v_cmp_lt_u32 vcc, v35, v70\n v_lshl_add_u32 v35, v35, 1, v71\n s_set_gpr_idx_off\n ds_read_u16 v7, v35\n" \
                  "s_ff1_i32_b32 s96, vcc_lo\n s_add_u32 s70, s70, s96\n s_cbranch_scc1 2f\n v_alignbit_b32 v32, v37, v36, s70\n" \
                  "s_waitcnt lgkmcnt(0)\n v_readlane_b32 s84, v7, s96\n s_bfe_u32 s85, s84, 0x6000a\n s_or_b32 s88, s85, s89\n" \
                  "v_mov_b32 v28, s84\n ds_write_b8 v8, v28\n v_add_u32 v8, 1, v8\n s_bfe_u32 s89, s84, s28\n"
// the next run: PFREE pending lanes again (what the copies in between did), the window back at its first bit
#define ENTRY_OLD(id) OLD_ENTRY RUN_FAST FIRST_LIT "s_mov_b32 s8, %3\n s_mov_b32 s70, -32\n"
#define ENTRY_NEW(id) NEW_ENTRY RUN_FAST FIRST_LIT "s_mov_b32 s8, %3\n s_mov_b32 s70, -32\n"

#define TIMED(NAME, BODY, PEND)                                                                                          \
    __global__ void NAME(u64 *out) {                                                                                     \
        __shared__ u32 lds[2560]; /* 10 KiB: 16 waves per CU; all zero: ring, info table, symbol lists */               \
        for (int k = threadIdx.x; k < 2560; k += 64) lds[k] = 0;                                                         \
        __syncthreads();                                                                                                 \
        u64 t0, t1;                                                                                                      \
        const u32 lane = threadIdx.x;                                                                                    \
        asm volatile("v_mov_b32 v1, %2\n v_sub_u32 v6, 32, %2\n v_and_b32 v12, 0xff, %2\n v_mov_b32 v23, 0\n v_mov_b32 v32, 0\n"   \
                     "v_mov_b32 v36, 0\n v_mov_b32 v37, 0\n v_mov_b32 v103, 0\n v_mov_b32 v71, 0\n v_mov_b32 v8, 0\n"    \
                     "v_cmp_eq_u32 vcc, 3, %2\n v_cndmask_b32 v70, 0, 1, vcc\n" /* tree 0: every code has 3 bits */      \
                     "s_mov_b32 s8, %3\n s_mov_b32 s9, 0\n s_mov_b32 s52, 64\n s_mov_b32 s53, 5\n s_mov_b32 s55, 0x7fffffff\n" \
                     "s_mov_b32 s65, 0x7fffffff\n s_mov_b32 s92, 0\n s_mov_b32 s70, -32\n s_mov_b32 s71, 0x3f\n s_mov_b32 s28, 0x20008\n" \
                     "s_mov_b32 s22, 0x20000\n s_mov_b32 s3, 3\n s_mov_b32 s95, %4\n s_mov_b64 exec, 0x1ffff\n"            \
                     "s_memtime %0\n s_waitcnt lgkmcnt(0)\n"                                                              \
                     "1:\n" BODY "s_sub_u32 s95, s95, 1\n s_cbranch_scc0 1b\n"                                           \
                     "s_memtime %1\n s_waitcnt lgkmcnt(0)\n 2:\n s_set_gpr_idx_off\n s_mov_b64 exec, -1\n"                  \
                     : "=s"(t0), "=s"(t1) : "v"(lane), "n"(PEND), "n"(ITERS - 1)                                          \
                     : "vcc", "scc", "memory", "m0", "s3", "s8", "s9", "s22", "s28", "s52", "s53", "s55", "s65", "s68", "s70", "s71",    \
                       "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s95", "s96", "v1", "v6", "v7", "v8", "v12", "v18",\
                       "v19", "v20", "v21", "v22", "v23", "v24", "v28", "v32", "v35", "v36", "v37", "v70", "v71", "v103");          \
        if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;                                                                  \
    }
TIMED(k_old_8, R16(ENTRY_OLD), 8)
TIMED(k_new_8, R16(ENTRY_NEW), 8)
TIMED(k_old_40, R16(ENTRY_OLD), 40)
TIMED(k_new_40, R16(ENTRY_NEW), 40)
TIMED(k_old_63, R16(ENTRY_OLD), 63)
TIMED(k_new_63, R16(ENTRY_NEW), 63)

int main() {
    const int full = 4096;
    u64 *o;
    if (hipMalloc(&o, full * sizeof(u64)) != hipSuccess) { printf("no device\n"); return 1; }
    std::vector<u64> h(full);
#define RUN(K, WHAT) { double r[2][2]; int w = 0; for (int waves : {1, full}) { double best = 1e30, worst = 0; for (int rep = 0; rep < 3; rep++) { \
        hipLaunchKernelGGL(K, dim3(waves), dim3(64), 0, 0, o); if (hipMemcpy(h.data(), o, waves * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); return 1; } \
        double sum = 0; for (int i = 0; i < waves; i++) sum += (double)h[i]; const double mean = sum / waves / (16.0 * ITERS); \
        if (mean < best) best = mean; if (mean > worst) worst = mean; } r[w][0] = best; r[w][1] = worst; w++; } \
      printf("%-58s lone wave %7.2f (%7.2f)   16 waves per CU %8.2f (%8.2f)\n", WHAT, r[0][0], r[0][1], r[1][0], r[1][1]); }
    printf("ticks per run entry (landing + first context + run bookkeeping + first literal): best of 3 launches (worst), mean over the launch's waves\n");
    RUN(k_old_8, "old: v_readlane + scalar fields,  8 pending lanes");
    RUN(k_new_8, "new: table read by the pending lanes + DPP,  8 lanes");
    RUN(k_old_40, "old, 40 pending lanes");
    RUN(k_new_40, "new, 40 pending lanes");
    RUN(k_old_63, "old, 63 pending lanes");
    RUN(k_new_63, "new, 63 pending lanes");
    return 0;
}
