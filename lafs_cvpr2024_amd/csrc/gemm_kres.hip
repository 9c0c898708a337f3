// K-resident streaming GEMM for gfx950:  C[M,N] = epilogue(A[M,384] * W[N,384]^T)
//
// Replaces the cuBLAS GEMMs behind Attention.qkv / Attention.proj / Mlp.fc1 (forward) and the input gradients of proj / fc2
// of the reference's ViT-S trunk (vision_transformer.py:59-65, 75-90): the five GEMM shapes of a block whose reduction axis is
// the embedding width.  lafs_gemm_nt (gemm.hip) dispatches here; everything else stays on the tiled kernel.
//
// Why another kernel (profiles/round2_*): at K = 384 the tiled kernel's 12-step main loop is bound by the
// L2 -> LDS request rate (612 MB of half-line LDS-DMA requests per fc1 GEMM: both operands re-staged per 256x128 tile), its
// epilogue by the HBM write rate, and the two phases add up (fc1: 52 + 58 us alone, 131-138 together) because a tile's stores
// leave as one burst per workgroup.  Here the token operand never touches the LDS and the stores never burst:
//   * a wave keeps its 32 token rows x all 384 k RESIDENT IN REGISTERS (two 16-row MFMA blocks, 96 VGPRs, loaded once per
//     128-row unit -- through the ring buffers, as four 32-row stages, while no weight stage is in flight) and walks along N;
//     only the weights stream through the LDS -- as whole contiguous rows (768 B: full cache lines), 32 rows = 24 KiB per ring
//     stage, 3 stages;  L2 -> LDS traffic per fc1 GEMM 407 MB for the weights, 34-55 MB for the rows;
//   * v_mfma_f32_16x16x32_bf16 computes C^T blocks (first operand = 16 weight rows, second = 16 tokens): 48 MFMAs per stage and
//     barrier.  A lane (token t, quarter q) ends up with 4 consecutive output columns per MFMA; the weight rows of a stage are
//     interleaved so that two MFMAs give it 8 consecutive bf16 columns: every store instruction writes 16 rows x 64 contiguous
//     bytes (the pattern the HBM write path sustains at full rate; 16-byte pieces scattered over 32 rows -- what a 32x32 MFMA
//     layout produces -- measured 1.8-2.6 TB/s);
//   * work = (128-row unit, 64-column block) items.  A workgroup (4 waves, 2 workgroups per CU, all resident at once) gets a
//     contiguous part of ONE unit's N / 64 column blocks wherever that fills the chip well enough: kres_partition below splits
//     every unit into the same `parts` parts whose sizes differ by at most one, as many as fit the 512 workgroup slots, and the
//     parts of a unit have consecutive ids (one XCD: they read the same rows out of its L2).  The resident rows are then loaded
//     once per workgroup.  Elsewhere (few parts of many items: N = 1152 on 197 units, anything on 345 units, more units than
//     slots) the unit-major item list is cut into equal contiguous runs, one per slot, and a run that reaches into a second unit
//     loads rows a second time.  Either way the rows are loaded in front of a unit's items, outside the item loop, with nothing
//     of the workgroup's own in flight but stores.  (Equal runs everywhere, with a least run length of 4 items that halved the
//     grid to 256 / 128 workgroups at the step's N = 384 launches, is what this replaces.)
//     An item is two ring stages (32 columns each) and one epilogue: the two stages' 64-byte pieces of a row are stored back to
//     back and complete 128-byte lines; a wave emits 4-8 stores per item, so the memory pipeline sees a steady trickle of stores
//     between the LDS-DMA requests instead of per-tile bursts;
//   * the accumulators of a stage start from the bias of their columns (LDS reads issued a phase ahead, straight into the
//     accumulator registers): the epilogue neither zero-fills nor adds a bias;
//   * the LDS-DMA ring runs across items with counted s_waitcnt vmcnt (loads and stores retire in issue order on gfx950, the
//     epilogue's memory operations are a compile-time count per item).
// The counted waits (NDMA = 6 LDS-DMA instructions per thread and stage, S stores and P operand loads per item):
//   row load     vmcnt(0) once the first three row stages are issued (it also covers the bias and DropPath-scale loads issued
//                behind them); vmcnt(2 NDMA) for the fourth row stage, the item's two weight stages being younger.  Unchanged
//                counts; what changed is that the load no longer sits inside the item loop, and that on a unit-aligned part its
//                vmcnt(0) drains nothing but itself.  The vmcnt(0) that stood in FRONT of a reload is gone: a unit's last item
//                leaves no stage in flight, and stores older than the row stages do not enter any count (a run's second unit: a
//                barrier alone frees the ring).
//   first stage  first item: vmcnt(NDMA) (younger: its second stage); later items: vmcnt(NDMA + S + P) (younger: the second stage
//                and the previous item's epilogue).  Unchanged.
//   second stage first item: vmcnt(NDMA) if a next item's stage was issued above, else vmcnt(0); later items: vmcnt(NDMA + S + P)
//                or vmcnt(S + P) on a unit's last item.  Unchanged.
#include <stdlib.h>
#include "common.hpp"
#include "gemm_plan.hpp"
#include "ctx.hpp"

namespace {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4v_t __attribute__((ext_vector_type(4)));

constexpr int KK = 384;                    // reduction length (compile-time: it sizes the register-resident operand)
constexpr int CPR = KK / 8;                // 16-byte chunks per weight row
constexpr int ROWB = KK * 2;               // bytes per weight row
constexpr int GROWS = 32;                  // weight rows per stage = output columns per step
constexpr int STAGE = GROWS * ROWB;        // 24 KiB
constexpr int NSTG = 3;
constexpr int NTH = 256;
constexpr int NDMA4 = STAGE / 16 / NTH;    // LDS-DMA instructions per thread and stage (6)
constexpr int NKK = KK / 32;               // k steps of a 16x16x32 MFMA (12)
constexpr int MAXN = 1536;                 // bias vector staged in LDS
constexpr int FD = 8;                      // fragment reads in flight ahead of their MFMAs
static_assert(CPR % 16 == 0 && STAGE % (16 * NTH) == 0, "stage layout");

struct KArgs {
  const bf16_t* A; const bf16_t* B;
  int M, N, lda, ldb;
  void* C; int ldc; void* C2; int ldc2;
  const float* bias; const float* resid; int ldr;
  const float* seq_scale; const int* row2seq;
  const bf16_t* aux; int ldaux;
  int cbn, units, parts;                   // 64-column blocks per row unit; 128-row units; parts a unit's blocks are split into (0: equal runs)
  int save_grad;                           // LAFS_GELU_SAVE_GRAD: GELU epilogue stores gelu'(u) for u / GELU' epilogue multiplies aux in as it is
};

// Which items a workgroup gets.  `slots` workgroups fit the chip at once (a multiple of 8).
//   parts > 0  every unit's cbn column blocks are split into `parts` contiguous parts -- the most that keep units * parts within
//              the slots; logical workgroup `id` takes part id % parts of unit id / parts: blocks [cbn * part / parts,
//              cbn * (part + 1) / parts).  The grid is rounded up to the 8 XCDs; the surplus workgroups find no unit.
//   parts == 0 equal contiguous runs of the unit-major item list over all the slots: items [items * id / grid, items * (id + 1) /
//              grid), which may reach into a second unit (a second row load).
// The choice: a part is ceil(cbn / parts) items and one row load; a run is items / slots items and, where it crosses a unit, two
// loads.  A row load costs about as much as 1.5 items (profiles/kres_unit_runs_ab.txt: 3 us per item with two workgroups on a CU,
// 3-6 us per reload), so parts win unless they leave so many slots empty that a part is 1.5 items longer than a run: N = 384 on
// 197 / 148 units takes 2 / 3 parts (394 x 3 / 444 x 2 items), N = 1152 on 148 units 3 parts (444 x 6), N = 1152 on 197 units
// (2 parts would be 9 items against runs of 6.9) and everything on 345 units (one part: 352 workgroups) stay on equal runs.
struct KresGrid { int parts, grid; };
inline KresGrid kres_partition(int units, int cbn, int slots) {
  int parts = slots / units;
  parts = parts > cbn ? cbn : parts;
  const long items = (long)units * cbn;
  if (parts < 1 || 2L * ((cbn + parts - 1) / parts) * slots > 2 * items + 3L * slots) return {0, slots};
  return {parts, (units * parts + 7) & ~7};
}

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void fence() { asm volatile("" ::: "memory"); }
__device__ __forceinline__ void st16(void* p, unsigned a, unsigned b, unsigned c, unsigned d) {
  const u32x4_t v = {a, b, c, d};
  *reinterpret_cast<u32x4_t*>(p) = v;
}
__device__ __forceinline__ void st16f(void* p, float a, float b, float c, float d) {
  const f32x4v_t v = {a, b, c, d};
  *reinterpret_cast<f32x4v_t*>(p) = v;
}

// memory operations of one item besides its LDS-DMA: S stores (active waves only) + P epilogue-operand loads
template <int EPI, bool HAS_U> struct EpiOps {
  static constexpr bool F32 = (EPI == LAFS_EPI_RESID_F32);
  static constexpr int S = F32 ? 8 : ((EPI == LAFS_EPI_BF16_GELU && HAS_U) ? 8 : 4);      // (HAS_U of the GELU' variants: see AUX_IS_GRAD)
  static constexpr int P = F32 ? 8 : ((EPI == LAFS_EPI_DGELU_BF16) ? 4 : 0);
};

template <int EPI, bool HAS_U>
__global__ __launch_bounds__(NTH, 2) void gemm_kres_kernel(KArgs p) {
  constexpr int UROWS = 128, NDMA = NDMA4;
  constexpr int S = EpiOps<EPI, HAS_U>::S, P = EpiOps<EPI, HAS_U>::P;
  constexpr bool F32 = EpiOps<EPI, HAS_U>::F32;
  // The epilogue operand is fetched within the item, a stage of MFMAs ahead of its use.  (Fetched one item ahead, GELU' spilled
  // beside the staged reload of the resident rows: no registers for a second operand buffer.)
  // GELU' variants: HAS_U = false means that aux already holds gelu'(u) (LAFS_GELU_SAVE_GRAD): no derivative math in the epilogue
  constexpr bool AUX_IS_GRAD = (EPI == LAFS_EPI_DGELU_BF16) && !HAS_U;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NSTG * STAGE];
  __shared__ __attribute__((aligned(16))) float sbias[MAXN];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = lane & 15, q = lane >> 4;
  // blocks b, b+8, ... share an XCD: give each XCD a contiguous run of ids (the parts of one row unit read the same A rows)
  const int G = (int)gridDim.x, per = G >> 3;
  const int id = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int cbn = p.cbn;
  int ib, ie;                                         // this workgroup's items in unit-major order (kres_partition)
  if (p.parts > 0) {
    const int part = id % p.parts, unit = id / p.parts;
    if (unit >= p.units) return;
    ib = unit * cbn + cbn * part / p.parts;
    ie = unit * cbn + cbn * (part + 1) / p.parts;
  } else {
    const long items = (long)p.units * cbn;
    ib = (int)(items * id / G);
    ie = (int)(items * (id + 1) / G);
    if (ie <= ib) return;
  }

  // LDS image of a stage: row rho (0..31) = 48 chunks; logical chunk c sits at chunk position c ^ (rho & 15) (conflict-free
  // ds_read_b128 of 16 rows x one chunk).  The image is lane-linear for the DMA, so the swizzle goes on the source column.
  // MFMA row s of 16-row group gi lands in lane quarter s >> 2, accumulator register s & 3.  bf16 outputs: the stage's weight
  // rows are interleaved (row = 8 (s >> 2) + 4 gi + (s & 3)) so that the two groups give a lane 8 consecutive columns; fp32
  // outputs: row = 16 gi + s (4 consecutive columns = 16 bytes per MFMA already).
  int doff[NDMA];
#pragma unroll
  for (int i = 0; i < NDMA; ++i) {
    const int x = i * NTH + tid, rho = x / CPR, cp = x % CPR, c = cp ^ (rho & 15);
    const int s16 = rho & 15, gi = rho >> 4;
    const int rowrel = F32 ? rho : (8 * (s16 >> 2) + 4 * gi + (s16 & 3));
    doff[i] = (rowrel * p.ldb + c * 8) * 2;           // bytes
  }
  // LDS-DMA from inline asm (common.hpp): with the builtin, hipcc's wait-count pass drains the whole DMA queue (vmcnt(0)) in
  // front of the first fragment read of every stage; the ring is counted by hand instead (wait_vm below)
  const unsigned lds0 = lds_addr_of(smem);
  int pstage = 0;                                     // ring buffer the next issued stage goes to
  auto issue = [&](int k) {                           // stage k: column block k >> 1, half k & 1
    const bf16_t* base = p.B + (size_t)(32 * k) * p.ldb;
    const unsigned st = lds0 + pstage * STAGE + wave * 1024;
    pstage = (pstage + 1 == NSTG) ? 0 : pstage + 1;
    fence();
#pragma unroll
    for (int i = 0; i < NDMA; ++i) lds_dma16_m0_s(base, (unsigned)doff[i], st + i * (NTH * 16));
    fence();
  };
  // The 32 token rows of wave `w` of unit `mu` as ONE ring stage (same 768-byte rows, same chunk swizzle as a weight stage):
  // LDS-DMA fetches whole rows (the per-lane gather of 16 rows x 64 bytes per instruction it replaces took ~7 us per reload,
  // bound by the CU's outstanding misses); the owning wave then reads its fragments with the weight-fragment addressing.
  auto issue_rows = [&](int mu, int w, int buf) {
    const unsigned st = lds0 + buf * STAGE + wave * 1024;
    fence();
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int x = i * NTH + tid, rho = x / CPR, cp = x % CPR, c = cp ^ (rho & 15);
      const int row = min(mu * UROWS + w * 32 + rho, p.M - 1);
      lds_dma16_m0(p.A + (size_t)row * p.lda + c * 8, st + i * (NTH * 16));
    }
    fence();
  };

  // fragment read offsets inside a stage: row 16 gi + t, chunk (4 kk + q) ^ t: four register offsets (kk & 3) + immediates
  int foff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    foff[i] = t * ROWB + (((4 * i + q) ^ t) << 4);
    asm volatile("" : "+v"(foff[i]));
  }
  bf16x8_t areg[2][NKK];                              // two 16-token blocks x 12 k steps: lane (t, q) holds k = 32 kk + 8 q .. + 7
  f32x4_t acc[2][2][2];                               // [stage of the item][weight row group][token block]
  uint4 pre[P > 0 ? P : 1];                           // epilogue operand of this item
  float sc[2] = {1.0f, 1.0f};
  bool active = false;
  int m0 = 0;

  auto fetch = [&](int cb, uint4 (&dst)[P > 0 ? P : 1]) {          // exactly P loads: the epilogue operand of column block cb
    if (P == 0) return;
    const int n0 = cb * 64;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int b = i & 1, x = i >> 1;                // bf16: x = stage; fp32: x = stage * 2 + row group
      const int mr = min(m0 + 16 * b, p.M - 1);
      if (F32) dst[i] = *reinterpret_cast<const uint4*>(p.resid + (size_t)mr * p.ldr + n0 + 16 * x + 4 * q);
      else dst[i] = *reinterpret_cast<const uint4*>(p.aux + (size_t)mr * p.ldaux + n0 + 32 * x + 8 * q);
    }
    fence();
  };
  // The accumulators of a stage start from the bias of their four columns (LDS reads issued a phase ahead -- before the wait and
  // barrier in front of the item's first stage, before the first stage's MFMAs for the second -- straight into the registers the
  // MFMAs accumulate in): no zero fill, no bias add, and no LDS latency exposed at the head of the epilogue.
  auto bias_init = [&](f32x4_t (&a)[2][2], int n0, int g) {
#pragma unroll
    for (int gi = 0; gi < 2; ++gi) {
      const int n = F32 ? n0 + 16 * (2 * g + gi) + 4 * q : n0 + 32 * g + 8 * q + 4 * gi;
#pragma unroll
      for (int b = 0; b < 2; ++b) a[gi][b] = *reinterpret_cast<const f32x4_t*>(sbias + n);
    }
  };
  auto mfma_stage = [&](int stage, f32x4_t (&a)[2][2]) {            // 48 MFMAs on one ring stage
    __builtin_amdgcn_sched_barrier(0);
    const unsigned char* st = smem + stage * STAGE;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
      for (int gi = 0; gi < 2; ++gi) {
        const bf16x8_t w = *reinterpret_cast<const bf16x8_t*>(st + foff[kk & 3] + (kk >> 2) * 256 + gi * (16 * ROWB));
        a[gi][0] = mfma16(w, areg[0][kk], a[gi][0]);
        a[gi][1] = mfma16(w, areg[1][kk], a[gi][1]);
      }
    // fragment reads run FD ahead of the MFMA pairs that consume them (hipcc on its own keeps one read in flight and exposes
    // the LDS latency 24 times per stage: 1440 instead of ~1000 cycles)
    // (12 in flight measured no better: the phase is not latency-bound any more)
    __builtin_amdgcn_sched_group_barrier(0x100, FD, 0);
#pragma unroll
    for (int i = 0; i < 2 * NKK - FD; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 2 * FD, 0);
    __builtin_amdgcn_sched_barrier(0);
  };

  auto read_rows = [&](int buf) {                     // this wave's 32 rows out of ring buffer `buf` into areg
    const unsigned char* st = smem + buf * STAGE;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk)
        areg[b][kk] = *reinterpret_cast<const bf16x8_t*>(st + foff[kk & 3] + (kk >> 2) * 256 + b * (16 * ROWB));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the reads have returned before the buffer is handed back at the barrier
  };
  const int mu0 = ib / cbn;
  for (int mu = mu0; mu * cbn < ie; ++mu) {
    // ---------------- the resident operand, once per unit and in front of its items.  The ring is free: nothing has been issued
    // yet, or (a run that reaches into a second unit) no stage is in flight after a unit's last item and every wave is through
    // with reading it.
    const bool first_unit = (mu == mu0);
    const int cb0 = max(ib - mu * cbn, 0), cb1 = min(ie - mu * cbn, cbn);          // the unit's column blocks of this workgroup
    m0 = mu * UROWS + wave * 32 + t;
    active = (mu * UROWS + wave * 32) < p.M;
    if (!first_unit) __builtin_amdgcn_s_barrier();
    issue_rows(mu, 0, 0); issue_rows(mu, 1, 1); issue_rows(mu, 2, 2);
    // the bias vector and the DropPath scales are fetched behind the row stages, under their latency
    if (first_unit)
      for (int i = tid; i < p.N; i += NTH) sbias[i] = p.bias ? p.bias[i] : 0.f;
    if (EPI == LAFS_EPI_RESID_F32 && p.seq_scale != nullptr) {
#pragma unroll
      for (int b = 0; b < 2; ++b) sc[b] = p.seq_scale[p.row2seq[min(m0 + 16 * b, p.M - 1)]];
    }
    wait_vm<0>();                                     // (also keeps the bias and scale loads out of the counted waits below)
    __syncthreads();
    if (wave < 3) read_rows(wave);
    __builtin_amdgcn_s_barrier();                     // buffers free again
    issue_rows(mu, 3, 0);
    pstage = 1;
    issue(2 * cb0);                                   // -> buffer 1
    issue(2 * cb0 + 1);                               // -> buffer 2; the stage after them goes to buffer 0
    wait_vm<2 * NDMA>();                              // wave 3's rows have landed (the two weight stages are younger)
    __builtin_amdgcn_s_barrier();
    if (wave == 3) read_rows(0);
    int stage = 1;                                    // ring buffer the next consumed stage sits in
    for (int cb = cb0; cb < cb1; ++cb) {
      const int k0 = 2 * cb;
      const bool first = (cb == cb0);                   // no epilogue operations of a previous item in flight
      const bool feed_next = (cb + 1 < cb1);            // the stages of the NEXT item are issued from this one
      bias_init(acc[0], cb * 64, 0);
      // ---------------- first stage of the item.  Younger than its DMA: the item's other stage, and the previous item's epilogue
      // operations.  (The barrier also hands buffer 0 back after wave 3's row read.)
      if (first) wait_vm<NDMA>();
      else if (active) wait_vm<NDMA + S + P>();
      else wait_vm<NDMA + P>();
      __builtin_amdgcn_s_barrier();
      if (feed_next) issue(k0 + 2);
      bias_init(acc[1], cb * 64, 1);
      mfma_stage(stage, acc[0]);
      stage = (stage + 1 == NSTG) ? 0 : stage + 1;
      // ---------------- second stage: younger than its DMA are the previous item's epilogue operations (none in the first item)
      // and the stage issued above (if any)
      if (first) {
        if (feed_next) wait_vm<NDMA>(); else wait_vm<0>();
      } else if (feed_next) {
        if (active) wait_vm<NDMA + S + P>(); else wait_vm<NDMA + P>();
      } else {
        if (active) wait_vm<S + P>(); else wait_vm<P>();
      }
      __builtin_amdgcn_s_barrier();
      if (feed_next) issue(k0 + 3);
      fetch(cb, pre);                                   // P loads, consumed a stage of MFMAs later
      mfma_stage(stage, acc[1]);
      stage = (stage + 1 == NSTG) ? 0 : stage + 1;

      // ---------------- epilogue: lane (t, q) owns rows m0 and m0 + 16 and, per row and stage, 8 consecutive columns (bf16 outputs:
      // both row groups) or 2 x 4 consecutive columns (fp32 outputs: one piece per row group).  The two stages' pieces of a row
      // are stored back to back: each pair completes 128-byte lines (one step apart they reached the HBM as separate half-line
      // writes: 1.28x write traffic, profiles/round2_kernel_pmc.json history).
      fence();
      const int n0 = cb * 64;
      if (active) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int m = m0 + 16 * b;
          const bool rowok = (m < p.M);
          if (F32) {
#pragma unroll
            for (int x = 0; x < 4; ++x) {                // x = stage * 2 + row group: 16 columns each
              const int g = x >> 1, gi = x & 1;
              const int n = n0 + 16 * x + 4 * q;
              const uint4 r4 = pre[x * 2 + b];
              float v0 = acc[g][gi][b][0], v1 = acc[g][gi][b][1], v2 = acc[g][gi][b][2], v3 = acc[g][gi][b][3];
              v0 = __uint_as_float(r4.x) + sc[b] * v0; v1 = __uint_as_float(r4.y) + sc[b] * v1;
              v2 = __uint_as_float(r4.z) + sc[b] * v2; v3 = __uint_as_float(r4.w) + sc[b] * v3;
              if (rowok) st16f(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n, v0, v1, v2, v3);
            }
          } else {
            float v[2][8];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
              v[g][0] = acc[g][0][b][0]; v[g][1] = acc[g][0][b][1]; v[g][2] = acc[g][0][b][2]; v[g][3] = acc[g][0][b][3];
              v[g][4] = acc[g][1][b][0]; v[g][5] = acc[g][1][b][1]; v[g][6] = acc[g][1][b][2]; v[g][7] = acc[g][1][b][3];
              if (EPI == LAFS_EPI_DGELU_BF16) {
                const uint4 a4 = pre[g * 2 + b];
                if constexpr (AUX_IS_GRAD) {               // aux already holds gelu'(u)
                  v[g][0] *= bf_lo(a4.x); v[g][1] *= bf_hi(a4.x); v[g][2] *= bf_lo(a4.y); v[g][3] *= bf_hi(a4.y);
                  v[g][4] *= bf_lo(a4.z); v[g][5] *= bf_hi(a4.z); v[g][6] *= bf_lo(a4.w); v[g][7] *= bf_hi(a4.w);
                } else {
                  v[g][0] *= gelu_grad_f(bf_lo(a4.x)); v[g][1] *= gelu_grad_f(bf_hi(a4.x)); v[g][2] *= gelu_grad_f(bf_lo(a4.y)); v[g][3] *= gelu_grad_f(bf_hi(a4.y));
                  v[g][4] *= gelu_grad_f(bf_lo(a4.z)); v[g][5] *= gelu_grad_f(bf_hi(a4.z)); v[g][6] *= gelu_grad_f(bf_lo(a4.w)); v[g][7] *= gelu_grad_f(bf_hi(a4.w));
                }
              }
            }
            float dv[2][8];                                // GELU epilogue saving gelu'(u): value and derivative from one exp / rcp
            const bool both = (EPI == LAFS_EPI_BF16_GELU) && HAS_U && p.save_grad;
            if (both) {
#pragma unroll
              for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int e = 0; e < 8; ++e) { float gv; gelu_both_f(v[g][e], gv, dv[g][e]); v[g][e] = gv; }
#pragma unroll
              for (int g = 0; g < 2; ++g) {
                const int n = n0 + 32 * g + 8 * q;
                if (rowok) st16(reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + n, pack_bf2(dv[g][0], dv[g][1]), pack_bf2(dv[g][2], dv[g][3]),
                                pack_bf2(dv[g][4], dv[g][5]), pack_bf2(dv[g][6], dv[g][7]));
              }
            }
            if ((EPI != LAFS_EPI_BF16_GELU || HAS_U) && !both) {
#pragma unroll
              for (int g = 0; g < 2; ++g) {
                const int n = n0 + 32 * g + 8 * q;
                if (rowok) st16(reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + n, pack_bf2(v[g][0], v[g][1]), pack_bf2(v[g][2], v[g][3]),
                                pack_bf2(v[g][4], v[g][5]), pack_bf2(v[g][6], v[g][7]));
              }
            }
            if (EPI == LAFS_EPI_BF16_GELU) {
              if (!both) {
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                  for (int e = 0; e < 8; ++e) v[g][e] = gelu_f(v[g][e]);
              }
#pragma unroll
              for (int g = 0; g < 2; ++g) {
                const int n = n0 + 32 * g + 8 * q;
                if (rowok) st16(reinterpret_cast<bf16_t*>(p.C2) + (size_t)m * p.ldc2 + n, pack_bf2(v[g][0], v[g][1]), pack_bf2(v[g][2], v[g][3]),
                                pack_bf2(v[g][4], v[g][5]), pack_bf2(v[g][6], v[g][7]));
              }
            }
          }
        }
      }
      fence();
    }
  }
}

template <int EPI, bool HAS_U>
int launch(const KArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((gemm_kres_kernel<EPI, HAS_U>), dim3(grid), dim3(NTH), 0, s, a);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

}  // namespace

bool lafs_kres_eligible(const lafs_gemm_nt_args* g, NtPlan* p) {
  // LAFS_OPT_KRES_MASK = bit mask of the epilogues routed here (1 plain, 2 GELU, 4 residual, 8 GELU'); 0 = tiled kernel everywhere.
  // Default 15 (whole step, one box, tools/lab/ab_env.sh: 16.95 ms against 17.22 with mask 7 and 17.57 with 0).
  const int mask = lafs_ctx_opt(g->ctx, LAFS_OPT_KRES_MASK);
  const int e = g->epilogue;
  const int bit = e == LAFS_EPI_BF16 ? 1 : (e == LAFS_EPI_BF16_GELU ? 2 : (e == LAFS_EPI_RESID_F32 ? 4 : (e == LAFS_EPI_DGELU_BF16 ? 8 : 0)));
  if (!(mask & bit)) return false;
  if (g->splits > 1 || g->operand_f16) return false;
  if (g->K != KK || g->N % 64 != 0 || g->N > MAXN || g->N < 64 || g->M < 2048) return false;
  if (g->drop_p > 0.f) return false;
  // (the operands' presence, strides and alignment are the contract plan() has checked -- all but the stride of an absent C, which
  // the contract leaves free: a GELU request without u keeps the kernel it always had)
  if (g->C == nullptr && g->ldc % 8 != 0) return false;
  // two 4-wave workgroups per CU: one residency wave, every workgroup on a part of one row unit or on an equal run (kres_partition).
  // (LAFS_OPT_KRES_MIN_ITEMS, the least run length that used to halve the grid, stays an accepted option and is not read.)
  const int g_comm_cus = lafs_ctx_opt(g->ctx, LAFS_OPT_COMM_CUS);
  int slots = 512;
  if (g_comm_cus > 0 && slots > 2 * (256 - g_comm_cus)) slots = (2 * (256 - g_comm_cus)) & ~7;   // CUs left to RCCL (LAFS_OPT_COMM_CUS)
  const KresGrid kg = kres_partition((g->M + 127) / 128, g->N / 64, slots);
  // an item is 128 rows x 64 columns; a ring stage holds 32 weight rows over the whole K
  p->info = {/*route*/ 1, /*tile_m*/ 128, /*tile_n*/ 64, /*stage_k*/ KK, /*threads*/ NTH, /*f16*/ 0, /*k_slices*/ 1, /*workgroups*/ kg.grid};
  p->kres_parts = kg.parts;
  return true;
}

int lafs_kres_launch(const lafs_gemm_nt_args* g, const NtPlan& p, hipStream_t stream) {
  const int e = g->epilogue;
  KArgs a;
  a.A = (const bf16_t*)g->A; a.B = (const bf16_t*)g->B; a.M = g->M; a.N = g->N; a.lda = g->lda; a.ldb = g->ldb;
  a.C = g->C; a.ldc = g->ldc; a.C2 = g->C2; a.ldc2 = g->ldc2;
  a.bias = (e == LAFS_EPI_DGELU_BF16) ? nullptr : g->bias;
  a.resid = g->resid; a.ldr = g->ldr; a.seq_scale = g->seq_scale; a.row2seq = g->row2seq;
  a.aux = (const bf16_t*)g->aux; a.ldaux = g->ldaux;
  a.cbn = g->N / 64;
  a.save_grad = (g->act == LAFS_GELU_SAVE_GRAD && (e == LAFS_EPI_BF16_GELU || e == LAFS_EPI_DGELU_BF16)) ? 1 : 0;
  a.units = (g->M + 127) / 128;
  a.parts = p.kres_parts;
  const int grid = p.info.workgroups;
  switch (e) {
    case LAFS_EPI_BF16: return launch<LAFS_EPI_BF16, true>(a, grid, stream);
    case LAFS_EPI_BF16_GELU:
      return g->C != nullptr ? launch<LAFS_EPI_BF16_GELU, true>(a, grid, stream) : launch<LAFS_EPI_BF16_GELU, false>(a, grid, stream);
    case LAFS_EPI_RESID_F32: return launch<LAFS_EPI_RESID_F32, true>(a, grid, stream);
    default:
      return a.save_grad ? launch<LAFS_EPI_DGELU_BF16, false>(a, grid, stream) : launch<LAFS_EPI_DGELU_BF16, true>(a, grid, stream);
  }
}
