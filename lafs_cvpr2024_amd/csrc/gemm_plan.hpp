// Internal interface between gemm.hip (lafs_gemm_nt: validation, plan, dispatch) and the two kernels it routes to besides its own
// tiled one: gemm_kres.hip (K-resident streaming kernel) and gemm_big.hip (one persistent workgroup per CU).
#pragma once
#include "lafs_hip.h"

// What lafs_gemm_nt launches for a request.  Made once, by plan() in gemm.hip; the launchers read it and decide nothing.
struct NtPlan {
  lafs_gemm_nt_plan_info info;     // route, tile, stage depth, threads, K slices, workgroups: what lafs_gemm_nt_plan reports
  int inst, klen;                  // tiled kernel: the gemm_nt_kernel instantiation (NtInst of gemm.hip), length of a K slice
  int geo;                         // gemm_big: 1 = 192 x 256, 2 = 256 x 256 (two waves per SIMD), 3 = 176 x 256, 4 = 160 x 256
  int kres_parts;                  // K-resident kernel: contiguous parts a row unit's column blocks are split into, one workgroup each
};

// *_eligible: whether this kernel is the one to run a request that plan() has VALIDATED (the measured shape and option thresholds
// live with the kernels); when true, *p holds the route, the tile and the grid.
//   K-resident: K == 384, N % 64 == 0, 64 <= N <= 1536, at least 2048 rows, plain / GELU / GELU' / residual epilogue, no dropout,
//   no K split (LAFS_OPT_KRES_MASK = 0 switches it off for A/B runs)
bool lafs_kres_eligible(const lafs_gemm_nt_args* g, NtPlan* p);
int lafs_kres_launch(const lafs_gemm_nt_args* g, const NtPlan& p, hipStream_t stream);
//   one workgroup per CU: bf16 operands, K % 64 == 0, K >= 512, wide outputs (N >= 512) on many rows, plain / GELU / GELU' /
//   residual epilogue, no K split, and expected to win (LAFS_OPT_NT_BIG = 0 switches it off for A/B runs)
bool lafs_big_eligible(const lafs_gemm_nt_args* g, NtPlan* p);
int lafs_big_launch(const lafs_gemm_nt_args* g, const NtPlan& p, hipStream_t stream);
