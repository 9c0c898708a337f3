// Host-side transformer engine: sequences the HIP kernels of one pre-LN ViT trunk (all blocks) over a packed
// token batch, forward and backward, with every activation in a caller-provided workspace.  One C call per
// trunk pass -> no per-op Python/dispatcher overhead, and the whole pass is hipGraph-capturable (no allocation,
// no synchronisation, only kernel launches on `stream`).
//
// Mirrors Block.forward (vision_transformer.py:107-113) / Residual_droppath(PreNorm(.)) (face_pre_pro/ViT_face.py:106-120):
//   x1 = x0 + s_a * proj(attn(LN1(x0)));   x0' = x1 + s_m * fc2(gelu(fc1(LN2(x1))))
// The residual stream is fp32; GEMM operands are bf16 (fp32 accumulate).
#include <algorithm>
#include <vector>
#include <stdlib.h>
#include "common.hpp"
#include "lafs_hip.h"
#include "ctx.hpp"

namespace {

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct LayerBuf {
  float* x0; float* st1; bf16_t* h1; bf16_t* qkv; float* lse; bf16_t* o; float* x1; float* st2; bf16_t* h2; bf16_t* u; bf16_t* a;
};
struct Scratch {             // operands of the weight gradients: two slots used by layer parity (the wgrad stream may lag one layer behind),
  std::vector<bf16_t*> gbm, gba, du, dqkv;   // or one slot per layer when the weight gradients are deferred (lafs_trunk_desc::wgrad_defer)
  bf16_t* dh; bf16_t* d_o;
};
inline int wg_slot(const lafs_trunk_desc* d, int l) { return d->wgrad_defer ? l : (l & 1); }
struct Carve {
  std::vector<LayerBuf> layers;   // depth entries when saving, 1 otherwise (reused)
  std::vector<float*> ln_part;    // [layer][norm 1 | 2][row chain 0..3]: per-workgroup gamma / beta sums of the LayerNorm backward
  float* ln_slot(int l, int norm2, int chain) const { return ln_part[((size_t)l * 2 + norm2) * 4 + chain]; }
  float* xalt;                    // ping-pong residual buffer for the no-save path
  // lafs_trunk_desc::cls_only_last (else NULL): the identity row -> sequence table of the compact cls rows (DropPath scales) and two
  // f32 [n_seq, dim] row sets (forward: the block input's cls rows | the block's output rows; backward: the gradient stream's)
  // and the cls attention's outputs o_c (bf16 [n_seq, inner]) | lse_c (f32 [n_seq, heads]): the row chains write them while other chains
  // may still run earlier blocks -- in a forward-only pass on the ONE buffer set all blocks share -- so they alias no dense buffer
  int32_t* seq_id; float* xc0; float* xc1; bf16_t* oc; float* lsec;
  Scratch s;
  void* wg_ws; size_t wg_bytes;   // slice partials of the grouped weight-gradient launch (lafs_wgrad_group)
  size_t bytes;
};
// floats of one LayerNorm slot buffer (lafs_layernorm_bwd part_out; lafs_layernorm_bwd_fold adds them in a fixed order)
size_t ln_slot_floats(const lafs_trunk_desc* d) {
  return (size_t)std::max(lafs_layernorm_bwd_parts(d->n_tok, d->dim), lafs_mlp_fused_ln_parts(d->n_tok)) * 2 * d->dim;
}

// the four weight gradients of one block as lafs_wgrad_group items (pointers filled in by the caller)
void block_wgrad_shapes(const lafs_trunk_desc* d, lafs_wgrad_item (&it)[4]) {
  const int D = d->dim, I = d->inner, M = d->mlp;
  for (auto& x : it) x = lafs_wgrad_item{};
  it[0].N1 = D; it[0].N2 = M; it[0].lda = D; it[0].ldb = M; it[0].ldc = M;              // fc2:  dW = gbm^T a
  it[1].N1 = M; it[1].N2 = D; it[1].lda = M; it[1].ldb = D; it[1].ldc = D;              // fc1:  dW = du^T h2
  it[2].N1 = D; it[2].N2 = I; it[2].lda = D; it[2].ldb = I; it[2].ldc = I;              // proj: dW = gba^T o
  it[3].N1 = 3 * I; it[3].N2 = D; it[3].lda = 3 * I; it[3].ldb = D; it[3].ldc = D;      // qkv:  dW = dqkv^T h1
}

Carve carve(const lafs_trunk_desc* d, void* ws, int save) {
  Carve c;
  unsigned char* base = reinterpret_cast<unsigned char*>(ws);
  size_t off = 0;
  const size_t T = (size_t)d->n_tok, D = d->dim, I = d->inner, M = d->mlp, H = d->heads;
  auto take = [&](size_t bytes) { unsigned char* p = base ? base + off : nullptr; off += al(bytes); return p; };
  const int nl = save ? d->depth : 1;
  c.layers.resize(nl);
  for (int l = 0; l < nl; ++l) {
    LayerBuf& b = c.layers[l];
    b.x0 = (l == 0) ? nullptr : (float*)take(T * D * 4);     // layer 0 reads the caller's x_in
    b.st1 = (float*)take(T * 2 * 4);
    b.h1 = (bf16_t*)take(T * D * 2);
    b.qkv = (bf16_t*)take(T * 3 * I * 2);
    b.lse = (float*)take(T * H * 4);
    b.o = (bf16_t*)take(T * I * 2);
    b.x1 = (float*)take(T * D * 4);
    b.st2 = (float*)take(T * 2 * 4);
    b.h2 = (bf16_t*)take(T * D * 2);
    b.u = (bf16_t*)take(T * M * 2);
    b.a = (bf16_t*)take(T * M * 2);
  }
  c.xalt = save ? nullptr : (float*)take(T * D * 4);
  c.seq_id = nullptr; c.xc0 = c.xc1 = nullptr; c.oc = nullptr; c.lsec = nullptr;
  if (d->cls_only_last) {
    c.seq_id = (int32_t*)take((size_t)d->n_seq * 4);
    c.xc0 = (float*)take((size_t)d->n_seq * D * 4);
    c.xc1 = (float*)take((size_t)d->n_seq * D * 4);
    c.oc = (bf16_t*)take((size_t)d->n_seq * I * 2);
    c.lsec = (float*)take((size_t)d->n_seq * H * 4);
  }
  if (save) {
    const int nslot = d->wgrad_defer ? d->depth : 2;
    c.s.gbm.resize(nslot); c.s.gba.resize(nslot); c.s.du.resize(nslot); c.s.dqkv.resize(nslot);
    for (int q = 0; q < nslot; ++q) {
      c.s.gbm[q] = (bf16_t*)take(T * D * 2);
      c.s.gba[q] = (bf16_t*)take(T * D * 2);
      c.s.du[q] = (bf16_t*)take(T * M * 2);
      c.s.dqkv[q] = (bf16_t*)take(T * 3 * I * 2);
    }
    c.s.dh = (bf16_t*)take(T * D * 2);
    c.s.d_o = (bf16_t*)take(T * I * 2);
    // (four full-size slot buffers per norm whatever the number of row chains in use -- 75 MB of 7.3 GB at C2: the chain count is an
    // option of the context, which may change on a live engine after its workspace was sized; sizing by the chains in use, as the
    // round-5 advisor suggested, would make that a silent overflow)
    c.ln_part.resize((size_t)d->depth * 2 * 4);
    for (auto& q : c.ln_part) q = (float*)take(ln_slot_floats(d) * 4);
    lafs_wgrad_item it[4];
    block_wgrad_shapes(d, it);
    // (the single-stream backward uses the whole chip: size for whichever plan needs more)
    int64_t wb = std::max(lafs_wgrad_group_workspace_bytes(it, 4, d->n_tok, d->wgrad_workgroups),
                          lafs_wgrad_group_workspace_bytes(it, 4, d->n_tok, 0));
    if (d->cls_only_last)     // the last block's two launches: fc2 / fc1 / proj over the n_seq cls rows, qkv over all rows
      for (int wg : {d->wgrad_workgroups, 0})
        wb = std::max({wb, lafs_wgrad_group_workspace_bytes(it, 3, d->n_seq, wg), lafs_wgrad_group_workspace_bytes(it + 3, 1, d->n_tok, wg)});
    c.wg_bytes = wb > 0 ? (size_t)wb : 0;
    c.wg_ws = take(c.wg_bytes > 0 ? c.wg_bytes : 256);
  } else {
    c.s = Scratch{};
    c.wg_ws = nullptr; c.wg_bytes = 0;
  }
  c.bytes = off;
  return c;
}

int check_desc(const lafs_trunk_desc* d) {
  LAFS_CHECK_ARG(d != nullptr, "null descriptor");
  LAFS_CHECK_ARG(d->dim > 0 && d->dim % 64 == 0 && d->mlp % 64 == 0 && d->inner == d->heads * 64, "dims must be multiples of 64");
  LAFS_CHECK_ARG(d->depth > 0 && d->n_tok > 0 && d->n_seq > 0 && d->max_len > 0 && d->max_len <= 256, "bad geometry");
  LAFS_CHECK_ARG(d->cu_seqlens && d->row2seq && d->master && d->shadow && d->blocks, "null pointer in descriptor");
  LAFS_CHECK_ARG(d->dropout_p >= 0.f && d->dropout_p < 1.f, "dropout_p must be in [0, 1)");
  LAFS_CHECK_ARG(d->n_groups >= 0 && d->n_groups <= 4, "at most 4 sequence groups");
  if (d->n_groups > 0) {
    int ns = 0;
    for (int gi = 0; gi < d->n_groups; ++gi) {
      LAFS_CHECK_ARG(d->group_n_seq[gi] > 0 && d->group_max_len[gi] > 0 && d->group_max_len[gi] <= d->max_len, "bad sequence group");
      ns += d->group_n_seq[gi];
    }
    LAFS_CHECK_ARG(ns == d->n_seq, "sequence groups must cover n_seq");
  }
  return LAFS_OK;
}

#define RUN(call)                        \
  do {                                   \
    const int rc_ = (call);              \
    if (rc_ != LAFS_OK) return rc_;      \
  } while (0)

// Side streams for the attention launches of the second and later crop-resolution groups and for the row chains: the 197-token and
// the 37-token launch of a layer are independent (both read the qkv GEMM's output, both feed the projection) and latency-bound on
// their own (profiles/round2_attention_pmc.txt: waves waiting 53-67 % of the time), so they run beside each other.  The streams and
// events belong to the descriptor's lafs_ctx (created with it, before anything is captured); without a context -- or with
// LAFS_OPT_SIDE_STREAMS = 0 -- everything stays on `stream`.
lafs_ctx* side_ctx(const lafs_trunk_desc* d) {
  lafs_ctx* c = d->ctx;
  return (c != nullptr && c->streams_ok && c->opt[LAFS_OPT_SIDE_STREAMS] != 0) ? c : nullptr;
}

// ---- The plan: everything the trunk passes branch on, decided once per call.  lafs_trunk_forward, lafs_trunk_backward and the
// LayerNorm fold at its end launch what it says; lafs_trunk_plan reports it (include/lafs_hip.h names the fields).
using Range = lafs_trunk_range_plan;

// The MLP launches of row range r.  The block's MLP is one launch (csrc/mlp_fused.hip) where the context's LAFS_OPT_MLP_FUSED
// asks for it and the geometry allows.
void plan_mlp(const lafs_trunk_desc* d, int save, Range& r) {
  const int opt = lafs_ctx_opt(d->ctx, LAFS_OPT_MLP_FUSED);
  const bool can = d->dropout_p == 0.f && lafs_mlp_fused_supported(d->dim, d->mlp, r.rows) != 0;
  auto on = [&](int bit) { return can && (opt & bit) != 0; };
  r.fwd_fused = on(save ? LAFS_MLP_FUSED_FWD_SAVE : LAFS_MLP_FUSED_FWD);
  r.fwd_ln2_inside = r.fwd_fused && on(LAFS_MLP_FUSED_LN2);
  // (not with the merged launch of MERGE_CHAINS, whose row count differs from the attention branch's: the bit switches it off)
  r.fwd_next_ln1 = r.fwd_fused && on(LAFS_MLP_FUSED_NEXT_LN1) && !(opt & LAFS_MLP_FUSED_MERGE_CHAINS);
  r.fwd_proj_inside = r.fwd_ln2_inside && d->inner == d->dim && on(save ? LAFS_MLP_FUSED_PROJ_FWD_SAVE : LAFS_MLP_FUSED_PROJ_FWD);
  r.bwd_fused = on(LAFS_MLP_FUSED_BWD);
  // (LayerNorm 2's gamma / beta slots are numbered by workgroup: one launch of no more units than a slot buffer holds)
  r.bwd_ln2_inside = r.bwd_fused && on(LAFS_MLP_FUSED_LN2_BWD) && (size_t)lafs_mlp_fused_ln_parts(r.rows) * 2 * d->dim <= ln_slot_floats(d);
  r.ln1_parts = lafs_layernorm_bwd_parts(r.rows, d->dim);
  r.ln2_parts = r.bwd_ln2_inside ? lafs_mlp_fused_ln_parts(r.rows) : r.ln1_parts;
}

// layer_hi: the pass covers blocks below it (a forward covers them all: depth)
int plan(const lafs_trunk_desc* d, int save, lafs_trunk_plan_info* p, int layer_hi) {
  RUN(check_desc(d));
  *p = lafs_trunk_plan_info{};
  // The last block on the cls rows alone (include/lafs_hip.h: cls_only_last).  Element-dropout masks are indexed by absolute row,
  // which a compacted row has lost; the deferred weight gradients (lafs_trunk_wgrad) read dense per-layer operand slots.
  p->cls_only_last = d->cls_only_last != 0 && d->dropout_p == 0.f && d->wgrad_defer == 0 && layer_hi == d->depth;
  p->whole = Range{0, d->n_tok, 0, 0, d->n_seq, 0};
  plan_mlp(d, save, p->whole);
  // Row ranges.  Nothing in a pass mixes token rows of different sequences: with two crop-resolution groups of full-length sequences
  // (element-dropout masks are indexed by absolute rows: drop_row0) the groups' rows run as independent chains of launches over
  // row sub-ranges of the same buffers, range i on stream i -- every kernel of a chain is latency-bound to some degree, and chains
  // side by side fill each other's gaps.  LAFS_OPT_ROW_CHAINS 1: one chain; 2: one per group; 4: half groups, cut at a sequence boundary.
  lafs_ctx* a = side_ctx(d);
  const int chains = a != nullptr ? a->opt[LAFS_OPT_ROW_CHAINS] : 1;
  auto rows = [&](int gi) { return d->group_n_seq[gi] * d->group_max_len[gi]; };
  if (chains >= 2 && d->n_groups == 2 && rows(0) + rows(1) == d->n_tok && rows(0) >= 4096 && rows(1) >= 4096) {
    const int parts = (chains == 4 && d->group_n_seq[0] >= 2 && d->group_n_seq[1] >= 2) ? 2 : 1;
    int row = 0, seq = 0;
    for (int gi = 0; gi < 2; ++gi) {
      const int ns = d->group_n_seq[gi], len = d->group_max_len[gi];
      for (int h = 0; h < parts; ++h) {
        const int q0 = ns * h / parts, q1 = ns * (h + 1) / parts;
        p->range[p->n_ranges] = Range{row + q0 * len, (q1 - q0) * len, gi, seq + q0, q1 - q0, p->n_ranges};
        plan_mlp(d, save, p->range[p->n_ranges++]);
      }
      row += ns * len; seq += ns;
    }
  } else {
    p->range[p->n_ranges++] = p->whole;
  }
  p->attention = d->n_groups <= 1 ? LAFS_ATTN_ONE_LAUNCH : (p->n_ranges == 1 && a != nullptr) ? LAFS_ATTN_PER_GROUP_FORKED : LAFS_ATTN_PER_GROUP;
  // MERGE_CHAINS (lab): the row chains meet in front of every MLP, which then runs as ONE launch over all rows -- whole rounds of the
  // chip plus a round of 64-row units instead of a round per chain (csrc/mlp_fused.hip); the projection stays with the chains
  p->mlp_merged = p->n_ranges > 1 && p->whole.fwd_fused && (lafs_ctx_opt(d->ctx, LAFS_OPT_MLP_FUSED) & LAFS_MLP_FUSED_MERGE_CHAINS) != 0;
  if (p->mlp_merged) {
    p->whole.fwd_proj_inside = 0;
    for (int i = 0; i < p->n_ranges; ++i) {
      Range& r = p->range[i];
      r.fwd_fused = 1; r.fwd_ln2_inside = p->whole.fwd_ln2_inside; r.fwd_next_ln1 = r.fwd_proj_inside = 0;
    }
  }
  return LAFS_OK;
}

int gemm(const lafs_ctx* cx, const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epi, void* C, int ldc, const float* bias,
         hipStream_t s, void* C2 = nullptr, int ldc2 = 0, const float* resid = nullptr, int ldr = 0,
         const float* seq_scale = nullptr, const int32_t* row2seq = nullptr, const void* aux = nullptr, int ldaux = 0,
         float drop_p = 0.f, uint32_t drop_seed = 0, int act = 0, const float* drop_step = nullptr, int drop_row0 = 0) {
  lafs_gemm_nt_args g = {};
  g.ctx = cx;
  g.drop_p = drop_p; g.drop_seed = drop_seed; g.act = act; g.drop_step = drop_step; g.drop_row0 = drop_row0;
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.epilogue = epi;
  g.C = C; g.ldc = ldc; g.C2 = C2; g.ldc2 = ldc2; g.bias = bias; g.resid = resid; g.ldr = ldr;
  g.seq_scale = seq_scale; g.row2seq = row2seq; g.aux = aux; g.ldaux = ldaux; g.splits = 1;
  return lafs_gemm_nt(&g, s);
}

#define HIP_TRY(call)                                                                         \
  do {                                                                                        \
    const hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                                   \
      lafs_set_error("%s:%d: %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_));      \
      return (int)e_;                                                                         \
    }                                                                                         \
  } while (0)
int side_fork(lafs_ctx* a, hipStream_t stream, int n) {          // n streams in all: `stream`, side[0 .. n - 2]
  HIP_TRY(hipEventRecord(a->fork, stream));
  for (int i = 0; i + 1 < n; ++i) HIP_TRY(hipStreamWaitEvent(a->side[i], a->fork, 0));
  return LAFS_OK;
}
int side_join(lafs_ctx* a, hipStream_t stream, int n) {
  for (int i = 0; i + 1 < n; ++i) {
    HIP_TRY(hipEventRecord(a->join[i], a->side[i]));
    HIP_TRY(hipStreamWaitEvent(stream, a->join[i], 0));
  }
  return LAFS_OK;
}
// Forked region: the first n_streams - 1 side streams see what `stream` has enqueued, body(0 .. n - 1) runs until one fails, and
// `stream` waits for the side streams.  The join is reached once a fork has been issued, also when the forked work failed: side
// streams left forked inside a hipGraph capture would make the capture fail later with an unrelated error.  Returns the first
// failure.  (n_streams < 2, or no side streams: the bodies alone.)
template <class Body>
int forked(const lafs_trunk_desc* d, hipStream_t stream, int n_streams, int n, Body&& body) {
  lafs_ctx* a = n_streams > 1 ? side_ctx(d) : nullptr;
  if (a != nullptr) RUN(side_fork(a, stream, n_streams));
  int rc = LAFS_OK;
  for (int i = 0; i < n && rc == LAFS_OK; ++i) rc = body(i);
  const int rc_join = a != nullptr ? side_join(a, stream, n_streams) : LAFS_OK;
  return rc != LAFS_OK ? rc : rc_join;
}

struct Pass {                     // one trunk pass: what the launches of every row range need
  const lafs_trunk_desc* d; const Carve& c; const lafs_trunk_plan_info& p; hipStream_t stream;
  int save;                                                            // forward: activations kept per layer
  const float* x_in; float* g;                                         // backward: layer 0's input, the gradient stream
  std::vector<const float*> lay_in; std::vector<float*> lay_out;       // forward: residual stream of every layer (the same for every row range)
  hipStream_t st(const Range& r) const { return r.stream == 0 ? stream : d->ctx->side[r.stream - 1]; }
  const int32_t* r2s(const Range& r) const { return d->row2seq + r.row0; }
  const float* scale(int l, int br) const { return d->drop_scales ? d->drop_scales + ((size_t)l * 2 + br) * d->n_seq : nullptr; }
  uint32_t seed(int l, int site) const { return d->dropout_seed + 3u * (uint32_t)l + (uint32_t)site; }   // sites: 0 to_out, 1 GELU, 2 fc2
};

// The attention launches of row range r in the plan's form: launch(cu_seqlens of the first sequence, sequences, longest, stream).
// (The attention kernels address tokens through cu_seqlens: base pointers, whatever the row range.)
template <class Launch>
int attention(const Pass& ps, const Range& r, Launch&& launch) {
  const lafs_trunk_desc* d = ps.d;
  hipStream_t st = ps.st(r);
  if (ps.p.attention == LAFS_ATTN_ONE_LAUNCH) return launch(d->cu_seqlens, d->n_seq, d->max_len, st);
  // one launch per crop resolution, each with its own tile shape; a range inside one group carries its own sequence count
  const bool fork = ps.p.attention == LAFS_ATTN_PER_GROUP_FORKED;
  const int ng = ps.p.n_ranges == 1 ? d->n_groups : 1;
  int s0[5] = {r.seq0};
  for (int k = 0; k < ng; ++k) s0[k + 1] = s0[k] + d->group_n_seq[r.group + k];
  return forked(d, st, fork ? 2 : 1, ng, [&](int k) {
    return launch(d->cu_seqlens + s0[k], ng == 1 ? r.n_seq : d->group_n_seq[r.group + k], d->group_max_len[r.group + k],
                  (fork && k > 0) ? d->ctx->side[0] : st);
  });
}

// ---- The last block on the cls rows (plan: cls_only_last).  Compact row i = sequence i; the compact activations live in the first
// n_seq rows of the layer's own buffers (x1, st2, h2, u, a: written on `stream` once the chains have joined) and of the weight-gradient
// operand slots; o_c / lse_c, which the chains write, have storage of their own (Carve::oc, lsec).
__global__ __launch_bounds__(256) void seq_id_kernel(int32_t* __restrict__ t, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = i;
}
int fill_seq_id(const Pass& ps) {
  hipLaunchKernelGGL(seq_id_kernel, dim3(ceil_div(ps.d->n_seq, 256)), dim3(256), 0, ps.stream, ps.c.seq_id, ps.d->n_seq);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

// Forward, per row chain: LayerNorm 1 and the qkv GEMM on every row (K and V are needed of every token), then the cls query's attention
int fwd_cls_chain(const Pass& ps, const Range& r) {
  const lafs_trunk_desc* d = ps.d;
  const int l = d->depth - 1;
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = ps.c.layers[ps.save ? l : 0];
  const int D = d->dim, I = d->inner, R = r.rows;
  const size_t rD = (size_t)r.row0 * D, rI = (size_t)r.row0 * I;
  const bf16_t* sh = reinterpret_cast<const bf16_t*>(d->shadow);
  hipStream_t st = ps.st(r);
  if (l == 0 || !r.fwd_next_ln1)
    RUN(lafs_layernorm_fwd(ps.lay_in[l] + rD, D, d->master + o.ln1_g, d->master + o.ln1_b, d->ln_eps, b.h1 + rD, D, nullptr, 0,
                           b.st1 + 2 * (size_t)r.row0, R, D, st));
  RUN(gemm(d->ctx, b.h1 + rD, D, sh + o.w_qkv, D, R, 3 * I, D, LAFS_EPI_BF16, b.qkv + 3 * rI, 3 * I, o.b_qkv >= 0 ? d->master + o.b_qkv : nullptr, st));
  return attention(ps, r, [&](const int32_t* cu, int nseq, int len, hipStream_t s) {
    const size_t s0 = (size_t)(cu - d->cu_seqlens);
    return lafs_attention_cls_fwd(b.qkv, 3 * I, cu, nseq, len, d->heads, d->attn_scale, ps.c.oc + s0 * I, I, ps.c.lsec + s0 * d->heads, s);
  });
}

// ... and, once the chains have joined, the row-local rest of the block on all n_seq cls rows at once (on `stream`)
int fwd_cls_rows(const Pass& ps) {
  const lafs_trunk_desc* d = ps.d;
  const int l = d->depth - 1;
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = ps.c.layers[ps.save ? l : 0];
  const Carve& c = ps.c;
  const int D = d->dim, I = d->inner, M = d->mlp, S = d->n_seq;
  const bf16_t* sh = reinterpret_cast<const bf16_t*>(d->shadow);
  hipStream_t st = ps.stream;
  RUN(fill_seq_id(ps));
  RUN(lafs_gather_cls(ps.lay_in[l], D, d->cu_seqlens, S, D, c.xc0, st));
  RUN(gemm(d->ctx, c.oc, I, sh + o.w_proj, I, S, D, I, LAFS_EPI_RESID_F32, b.x1, D, d->master + o.b_proj, st, nullptr, 0, c.xc0, D, ps.scale(l, 0),
           c.seq_id));
  RUN(lafs_layernorm_fwd(b.x1, D, d->master + o.ln2_g, d->master + o.ln2_b, d->ln_eps, b.h2, D, nullptr, 0, b.st2, S, D, st));
  RUN(gemm(d->ctx, b.h2, D, sh + o.w_fc1, D, S, M, D, LAFS_EPI_BF16_GELU, ps.save ? b.u : nullptr, M, d->master + o.b_fc1, st, b.a, M, nullptr, 0,
           nullptr, nullptr, nullptr, 0, 0.f, 0u, LAFS_GELU_SAVE_GRAD));
  RUN(gemm(d->ctx, b.a, M, sh + o.w_fc2, M, S, D, M, LAFS_EPI_RESID_F32, c.xc1, D, d->master + o.b_fc2, st, nullptr, 0, b.x1, D, ps.scale(l, 1),
           c.seq_id));
  return lafs_scatter_cls(c.xc1, d->cu_seqlens, S, D, ps.lay_out[l], D, st);
}

// Backward, on `stream` in front of the chains: the cls rows of g through the MLP, LayerNorm 2 and the projection
int bwd_cls_rows(const Pass& ps) {
  const lafs_trunk_desc* d = ps.d;
  const int l = d->depth - 1;
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = ps.c.layers[l];
  const Carve& c = ps.c;
  const Scratch& s = c.s;
  const int p = wg_slot(d, l), D = d->dim, I = d->inner, M = d->mlp, S = d->n_seq;
  const bf16_t* sht = reinterpret_cast<const bf16_t*>(d->shadow_t);
  hipStream_t st = ps.stream;
  // (c.seq_id: the identity table the forward of this workspace wrote)
  RUN(lafs_gather_cls(ps.g, D, d->cu_seqlens, S, D, c.xc0, st));
  RUN(lafs_scale_cast_bf16(c.xc0, D, s.gbm[p], D, ps.scale(l, 1), c.seq_id, S, D, 0.f, 0u, nullptr, 0, st));
  RUN(gemm(d->ctx, s.gbm[p], D, sht + o.w_fc2_t, D, S, M, D, LAFS_EPI_DGELU_BF16, s.du[p], M, nullptr, st, nullptr, 0, nullptr, 0, nullptr, nullptr,
           b.u, M, 0.f, 0u, LAFS_GELU_SAVE_GRAD));
  RUN(gemm(d->ctx, s.du[p], M, sht + o.w_fc1_t, M, S, D, M, LAFS_EPI_BF16, s.dh, D, nullptr, st));
  RUN(lafs_layernorm_bwd(s.dh, D, nullptr, 0, b.x1, D, b.st2, d->master + o.ln2_g, c.xc0, D, 1, s.gba[p], D, ps.scale(l, 0), c.seq_id,
                         d->grad + o.ln2_g, d->grad + o.ln2_b, S, D, 0.f, 0u, nullptr, 0, c.ln_slot(l, 1, 0), st));
  RUN(gemm(d->ctx, s.gba[p], D, sht + o.w_proj_t, D, S, I, D, LAFS_EPI_BF16, s.d_o, I, nullptr, st));
  return lafs_scatter_cls(c.xc0, d->cu_seqlens, S, D, ps.g, D, st);
}

// ... then per row chain: the cls query's attention backward fills the chain's whole dqkv range (dK, dV; dQ zero off the cls rows)
int bwd_cls_chain(const Pass& ps, const Range& r) {
  const lafs_trunk_desc* d = ps.d;
  const int l = d->depth - 1, I = d->inner;
  const LayerBuf& b = ps.c.layers[l];
  const Scratch& s = ps.c.s;
  bf16_t* dqkv = s.dqkv[wg_slot(d, l)];
  return attention(ps, r, [&](const int32_t* cu, int nseq, int len, hipStream_t as) {
    const size_t s0 = (size_t)(cu - d->cu_seqlens);
    return lafs_attention_cls_bwd(b.qkv, 3 * I, ps.c.oc + s0 * I, I, s.d_o + s0 * I, I, ps.c.lsec + s0 * d->heads, cu, nseq, len, d->heads, d->attn_scale,
                                  dqkv, 3 * I, as);
  });
}

// Forward of layer l over row range r, attention branch: LayerNorm 1 .. projection + residual
int fwd_attn_branch(const Pass& ps, const Range& r, int l) {
  const lafs_trunk_desc* d = ps.d;
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = ps.c.layers[ps.save ? l : 0];
  const int D = d->dim, I = d->inner, R = r.rows;
  const size_t rD = (size_t)r.row0 * D, rI = (size_t)r.row0 * I;
  const bf16_t* sh = reinterpret_cast<const bf16_t*>(d->shadow);
  const float* cur = ps.lay_in[l];
  hipStream_t st = ps.st(r);
  // (with fwd_next_ln1 the previous layer's fused MLP produced it: its epilogue holds the finished rows in registers)
  if (l == 0 || !r.fwd_next_ln1)
    RUN(lafs_layernorm_fwd(cur + rD, D, d->master + o.ln1_g, d->master + o.ln1_b, d->ln_eps, b.h1 + rD, D, nullptr, 0, b.st1 + 2 * (size_t)r.row0,
                           R, D, st));
  RUN(gemm(d->ctx, b.h1 + rD, D, sh + o.w_qkv, D, R, 3 * I, D, LAFS_EPI_BF16, b.qkv + 3 * rI, 3 * I, o.b_qkv >= 0 ? d->master + o.b_qkv : nullptr, st));
  RUN(attention(ps, r, [&](const int32_t* cu, int nseq, int len, hipStream_t s) {
    return lafs_attention_fwd(b.qkv, 3 * I, cu, nseq, len, d->heads, d->attn_scale, b.o, I, b.lse, s);
  }));
  if (!r.fwd_proj_inside)
    RUN(gemm(d->ctx, b.o + rI, I, sh + o.w_proj, I, R, D, I, LAFS_EPI_RESID_F32, b.x1 + rD, D, d->master + o.b_proj, st, nullptr, 0, cur + rD, D,
             ps.scale(l, 0), ps.r2s(r), nullptr, 0, d->dropout_p, ps.seed(l, 0), 0, d->dropout_step, r.row0));
  return LAFS_OK;
}

// ... and its MLP branch: LayerNorm 2 .. fc2 + residual
int fwd_mlp_branch(const Pass& ps, const Range& r, int l) {
  const lafs_trunk_desc* d = ps.d;
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = ps.c.layers[ps.save ? l : 0];
  const int D = d->dim, I = d->inner, M = d->mlp, R = r.rows;
  const size_t rD = (size_t)r.row0 * D, rI = (size_t)r.row0 * I, rM = (size_t)r.row0 * M;
  const bf16_t* sh = reinterpret_cast<const bf16_t*>(d->shadow);
  const float* cur = ps.lay_in[l];
  float* nxt = ps.lay_out[l];
  const float* sm = ps.scale(l, 1);
  hipStream_t st = ps.st(r);
  if (!r.fwd_ln2_inside)
    RUN(lafs_layernorm_fwd(b.x1 + rD, D, d->master + o.ln2_g, d->master + o.ln2_b, d->ln_eps, b.h2 + rD, D, nullptr, 0, b.st2 + 2 * (size_t)r.row0,
                           R, D, st));
  // a forward-only pass (teacher) never reads the pre-activation u: skip its store (77 MB per layer at C2).  A saving pass
  // stores gelu'(u) in its place (LAFS_GELU_SAVE_GRAD): that is all the backward needs of u, and the GELU' input gradient
  // becomes one multiply per value
  if (!r.fwd_fused) {
    RUN(gemm(d->ctx, b.h2 + rD, D, sh + o.w_fc1, D, R, M, D, LAFS_EPI_BF16_GELU, ps.save ? b.u + rM : nullptr, M, d->master + o.b_fc1, st,
             b.a + rM, M, nullptr, 0, nullptr, nullptr, nullptr, 0, d->dropout_p, ps.seed(l, 1), LAFS_GELU_SAVE_GRAD, d->dropout_step, r.row0));
    return gemm(d->ctx, b.a + rM, M, sh + o.w_fc2, M, R, D, M, LAFS_EPI_RESID_F32, nxt + rD, D, d->master + o.b_fc2, st, nullptr, 0, b.x1 + rD, D, sm,
                ps.r2s(r), nullptr, 0, d->dropout_p, ps.seed(l, 2), 0, d->dropout_step, r.row0);
  }
  lafs_mlp_args m = {};                                      // fc1 -> GELU -> fc2 -> residual in one launch, the hidden tile on chip
  m.X = b.h2 + rD; m.ldx = D; m.Wa = sh + o.w_fc1; m.ldwa = D; m.Wb = sh + o.w_fc2; m.ldwb = M; m.M = R; m.H = M;
  m.mode = ps.save ? LAFS_MLP_FWD_SAVE : LAFS_MLP_FWD;
  m.bias_a = d->master + o.b_fc1; m.bias_b = d->master + o.b_fc2; m.resid = b.x1 + rD; m.ldr = D; m.seq_scale = sm; m.row2seq = ps.r2s(r);
  m.out = nxt + rD; m.ldo = D;
  if (ps.save) { m.save_grad = b.u + rM; m.ldsg = M; m.save_act = b.a + rM; m.ldsa = M; }
  if (r.fwd_ln2_inside) {                                    // LayerNorm 2 as the fused kernel's prologue (no launch, no h2 round trip)
    m.X = nullptr; m.ln_gamma = d->master + o.ln2_g; m.ln_beta = d->master + o.ln2_b; m.ln_eps = d->ln_eps;
    if (ps.save) { m.ln_stats = b.st2 + 2 * (size_t)r.row0; m.ln_out = b.h2 + rD; m.ldln = D; }
  }
  if (r.fwd_proj_inside) {                                   // x1 = cur + sa * (o Wproj^T + b) is computed (and stored to b.x1) by this launch
    m.proj_x = b.o + rI; m.ldpx = I; m.proj_w = sh + o.w_proj; m.ldpw = I; m.proj_bias = d->master + o.b_proj;
    m.proj_resid = cur + rD; m.ldpr = D; m.proj_scale = ps.scale(l, 0);
  }
  if (l + 1 < d->depth && r.fwd_next_ln1) {                  // the next block's LayerNorm 1, from the rows in this launch's registers
    const lafs_block_offsets& on = d->blocks[l + 1];
    const LayerBuf& bn = ps.c.layers[ps.save ? l + 1 : 0];
    m.next_ln_gamma = d->master + on.ln1_g; m.next_ln_beta = d->master + on.ln1_b; m.next_ln_eps = d->ln_eps;
    m.next_ln_out = bn.h1 + rD; m.ldnln_next = D;
    m.next_ln_stats = ps.save ? bn.st1 + 2 * (size_t)r.row0 : nullptr;
  }
  m.ctx = d->ctx;
  return lafs_mlp_fused(&m, st);
}

// Backward of layer l over row range r, first part: from the GELU' input gradient to the attention backward
int bwd_head(const Pass& ps, const Range& r, int l) {
  const lafs_trunk_desc* d = ps.d;
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = ps.c.layers[l];
  const Scratch& s = ps.c.s;
  const int p = wg_slot(d, l), D = d->dim, I = d->inner, M = d->mlp, R = r.rows;
  const size_t rD = (size_t)r.row0 * D, rI = (size_t)r.row0 * I, rM = (size_t)r.row0 * M;
  const bf16_t* sht = reinterpret_cast<const bf16_t*>(d->shadow_t);
  hipStream_t st = ps.st(r);
  // ---- MLP branch ----
  if (r.bwd_fused) {                                         // GELU' input gradient -> fc1 input gradient in one launch (du written once)
    lafs_mlp_args m = {};
    m.X = s.gbm[p] + rD; m.ldx = D; m.Wa = sht + o.w_fc2_t; m.ldwa = D; m.Wb = sht + o.w_fc1_t; m.ldwb = M; m.M = R; m.H = M;
    m.mode = LAFS_MLP_BWD; m.out = s.dh + rD; m.ldo = D; m.save_grad = b.u + rM; m.ldsg = M; m.save_act = s.du[p] + rM; m.ldsa = M;
    m.ctx = d->ctx;
    if (r.bwd_ln2_inside) {                                  // LayerNorm 2's backward inside the same launch
      m.resid = b.x1 + rD; m.ldr = D; m.ln_stats = b.st2 + 2 * (size_t)r.row0; m.ln_gamma = d->master + o.ln2_g;
      m.ln_g_io = ps.g + rD; m.ldgio = D; m.ln_gb_out = s.gba[p] + rD; m.ldgb = D; m.seq_scale = ps.scale(l, 0); m.row2seq = ps.r2s(r);
      m.ln_part_out = ps.c.ln_slot(l, 1, r.stream);
    }
    RUN(lafs_mlp_fused(&m, st));
  } else {
    RUN(gemm(d->ctx, s.gbm[p] + rD, D, sht + o.w_fc2_t, D, R, M, D, LAFS_EPI_DGELU_BF16, s.du[p] + rM, M, nullptr, st, nullptr, 0, nullptr, 0, nullptr,
             nullptr, b.u + rM, M, d->dropout_p, ps.seed(l, 1), LAFS_GELU_SAVE_GRAD, d->dropout_step, r.row0));
    RUN(gemm(d->ctx, s.du[p] + rM, M, sht + o.w_fc1_t, M, R, D, M, LAFS_EPI_BF16, s.dh + rD, D, nullptr, st));
  }
  if (!r.bwd_ln2_inside)
    RUN(lafs_layernorm_bwd(s.dh + rD, D, nullptr, 0, b.x1 + rD, D, b.st2 + 2 * (size_t)r.row0, d->master + o.ln2_g, ps.g + rD, D, 1, s.gba[p] + rD, D,
                           ps.scale(l, 0), ps.r2s(r), d->grad + o.ln2_g, d->grad + o.ln2_b, R, D, d->dropout_p, ps.seed(l, 0), d->dropout_step,
                           r.row0, ps.c.ln_slot(l, 1, r.stream), st));
  // ---- attention branch ----
  RUN(gemm(d->ctx, s.gba[p] + rD, D, sht + o.w_proj_t, D, R, I, D, LAFS_EPI_BF16, s.d_o + rI, I, nullptr, st));
  return attention(ps, r, [&](const int32_t* cu, int nseq, int len, hipStream_t as) {
    return lafs_attention_bwd(b.qkv, 3 * I, b.o, I, s.d_o, I, b.lse, cu, nseq, len, d->heads, d->attn_scale, s.dqkv[p], 3 * I, as);
  });
}

// ... and second part: from the qkv input gradient to the LayerNorm backward that produces layer l-1's upstream gradient gbm[(l-1)&1]
int bwd_tail(const Pass& ps, const Range& r, int l) {
  const lafs_trunk_desc* d = ps.d;
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = ps.c.layers[l];
  const Scratch& s = ps.c.s;
  const float* x0 = (l == 0) ? ps.x_in : b.x0;
  const int p = wg_slot(d, l), D = d->dim, I = d->inner, R = r.rows;
  const bool more = l > 0;
  const size_t rD = (size_t)r.row0 * D, rI = (size_t)r.row0 * I;
  const bf16_t* sht = reinterpret_cast<const bf16_t*>(d->shadow_t);
  hipStream_t st = ps.st(r);
  RUN(gemm(d->ctx, s.dqkv[p] + 3 * rI, 3 * I, sht + o.w_qkv_t, 3 * I, R, D, 3 * I, LAFS_EPI_BF16, s.dh + rD, D, nullptr, st));
  return lafs_layernorm_bwd(s.dh + rD, D, nullptr, 0, x0 + rD, D, b.st1 + 2 * (size_t)r.row0, d->master + o.ln1_g, ps.g + rD, D, 1,
                            more ? s.gbm[wg_slot(d, l - 1)] + rD : nullptr, D, more ? ps.scale(l - 1, 1) : nullptr, ps.r2s(r), d->grad + o.ln1_g,
                            d->grad + o.ln1_b, R, D, more ? d->dropout_p : 0.f, more ? ps.seed(l - 1, 2) : 0u, d->dropout_step, r.row0,
                            ps.c.ln_slot(l, 0, r.stream), st);
}

}  // namespace

extern "C" int64_t lafs_trunk_workspace_bytes(const lafs_trunk_desc* d, int save_for_backward) {
  if (check_desc(d) != LAFS_OK) return -1;
  return (int64_t)carve(d, nullptr, save_for_backward).bytes;
}

extern "C" int lafs_trunk_plan(const lafs_trunk_desc* d, int save_for_backward, lafs_trunk_plan_info* out) {
  LAFS_CHECK_ARG(out != nullptr, "null plan");
  return plan(d, save_for_backward, out, d != nullptr ? d->depth : 0);
}

extern "C" int lafs_trunk_plan_layers(const lafs_trunk_desc* d, int save_for_backward, int layer_hi, int layer_lo, lafs_trunk_plan_info* out) {
  LAFS_CHECK_ARG(out != nullptr, "null plan");
  RUN(check_desc(d));
  LAFS_CHECK_ARG(0 <= layer_lo && layer_lo < layer_hi && layer_hi <= d->depth, "bad layer range");
  return plan(d, save_for_backward, out, layer_hi);
}

extern "C" int lafs_trunk_row_ranges(const lafs_trunk_desc* d) {
  lafs_trunk_plan_info p;
  return plan(d, 0, &p, d != nullptr ? d->depth : 0) == LAFS_OK ? p.n_ranges : -1;
}

extern "C" int lafs_trunk_forward(const lafs_trunk_desc* d, const float* x_in, float* x_out, void* workspace,
                                  int save_for_backward, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  lafs_trunk_plan_info p;
  RUN(plan(d, save_for_backward, &p, d != nullptr ? d->depth : 0));
  LAFS_CHECK_ARG(x_in && x_out && workspace, "null buffer");
  const Carve c = carve(d, workspace, save_for_backward);
  Pass ps{d, c, p, stream, save_for_backward, x_in, nullptr, std::vector<const float*>(d->depth), std::vector<float*>(d->depth)};
  const float* cur = x_in;
  for (int l = 0; l < d->depth; ++l) {
    float* nxt;
    if (l == d->depth - 1) nxt = x_out;
    else if (save_for_backward) nxt = c.layers[l + 1].x0;
    else nxt = (cur == c.xalt) ? x_out : c.xalt;            // ping-pong; never aliases x_in
    ps.lay_in[l] = cur; ps.lay_out[l] = nxt; cur = nxt;
  }
  const int dense = p.cls_only_last ? d->depth - 1 : d->depth;      // blocks that run on every row
  if (!p.mlp_merged) {        // every range runs all layers on its stream; the side streams join behind everything `stream` has enqueued
    RUN(forked(d, stream, p.n_ranges, p.n_ranges, [&](int i) {
      for (int l = 0; l < dense; ++l) {
        RUN(fwd_attn_branch(ps, p.range[i], l));
        RUN(fwd_mlp_branch(ps, p.range[i], l));
      }
      if (p.cls_only_last) RUN(fwd_cls_chain(ps, p.range[i]));
      return LAFS_OK;
    }));
  } else {
    for (int l = 0; l < dense; ++l) {
      RUN(forked(d, stream, p.n_ranges, p.n_ranges, [&](int i) { return fwd_attn_branch(ps, p.range[i], l); }));
      RUN(fwd_mlp_branch(ps, p.whole, l));
    }
    if (p.cls_only_last) RUN(forked(d, stream, p.n_ranges, p.n_ranges, [&](int i) { return fwd_cls_chain(ps, p.range[i]); }));
  }
  return p.cls_only_last ? fwd_cls_rows(ps) : LAFS_OK;
}

// The block's four weight gradients: ONE grouped launch, once all their operands exist.  Its 48 (ViT-S) output tiles x 5 token
// slices fill the chip together: 4x fewer slices -> 4x less partial-sum traffic than four separate launches (csrc/wgrad.hip)
// (cls_rows: the last block under the plan's cls_only_last -- fc2 / fc1 / proj sum over the n_seq compact rows of the same buffers, qkv
// over all rows: two launches, in order on the one stream that owns the slice workspace)
static int block_wgrad(const lafs_trunk_desc* d, const Carve& c, int l, int max_wg, hipStream_t st, bool cls_rows = false) {
  const lafs_block_offsets& o = d->blocks[l];
  const LayerBuf& b = c.layers[l];
  const Scratch& s = c.s;
  const int p = wg_slot(d, l);
  float* gr = d->grad;
  lafs_wgrad_item it[4];
  block_wgrad_shapes(d, it);
  it[0].A = s.gbm[p]; it[0].B = b.a; it[0].C = gr + o.w_fc2; it[0].colsum_a = gr + o.b_fc2;
  it[1].A = s.du[p]; it[1].B = b.h2; it[1].C = gr + o.w_fc1; it[1].colsum_a = gr + o.b_fc1;
  it[2].A = s.gba[p]; it[2].B = b.o; it[2].C = gr + o.w_proj; it[2].colsum_a = gr + o.b_proj;
  it[3].A = s.dqkv[p]; it[3].B = b.h1; it[3].C = gr + o.w_qkv; it[3].colsum_a = o.b_qkv >= 0 ? gr + o.b_qkv : nullptr;
  for (auto& x : it) x.accumulate = d->wgrad_overwrite ? 0 : 1;
  if (cls_rows) {
    it[2].B = c.oc;
    RUN(lafs_wgrad_group(it, 3, d->n_seq, max_wg, c.wg_ws, (int64_t)c.wg_bytes, st));
    return lafs_wgrad_group(it + 3, 1, d->n_tok, max_wg, c.wg_ws, (int64_t)c.wg_bytes, st);
  }
  return lafs_wgrad_group(it, 4, d->n_tok, max_wg, c.wg_ws, (int64_t)c.wg_bytes, st);
}

extern "C" int lafs_trunk_backward(const lafs_trunk_desc* d, const float* x_in, float* g, void* workspace, int layer_hi,
                                   int layer_lo, hipStream_t wgrad_stream, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  lafs_trunk_plan_info p;
  RUN(check_desc(d));
  LAFS_CHECK_ARG(0 <= layer_lo && layer_lo < layer_hi && layer_hi <= d->depth, "bad layer range");
  RUN(plan(d, 1, &p, layer_hi));
  LAFS_CHECK_ARG(x_in && g && workspace && d->shadow_t && d->grad, "null buffer");
  const Carve c = carve(d, workspace, 1);
  const Pass ps{d, c, p, stream, 1, x_in, g};
  const bool defer = d->wgrad_defer != 0;     // no weight-gradient launches here: lafs_trunk_wgrad issues them later from the per-layer slots
  // (the two-stream protocol takes its events from the context's pool: without a context the weight gradients stay on `stream`)
  const bool two = !defer && (wgrad_stream != nullptr) && (wgrad_stream != stream) && d->ctx != nullptr && d->ctx->streams_ok;
  hipStream_t s2 = two ? wgrad_stream : stream;
  const int nl = layer_hi - layer_lo;
  static std::vector<hipEvent_t> no_events;
  std::vector<hipEvent_t>& ev = two ? d->ctx->pool : no_events;
  LAFS_CHECK_ARG(!two || ev.size() >= (size_t)2 * nl + 1, "the context's event pool is too small for this layer range");
  int evi = 0;
  bool ev_failed = false;                  // a failed event call of the two-stream protocol (reported at the end of the call)
  auto fork = [&]() {                      // work enqueued on s2 after this sees everything enqueued on `stream` so far
    if (!two) return;
    hipEvent_t e = ev[evi++];
    if (hipEventRecord(e, stream) != hipSuccess || hipStreamWaitEvent(s2, e, 0) != hipSuccess) ev_failed = true;
  };
  std::vector<hipEvent_t> done(d->depth, nullptr);
  const bool cls = p.cls_only_last != 0;      // (layer_hi == depth) the first block of this walk runs on the cls rows behind its qkv GEMM
  if (cls) RUN(bwd_cls_rows(ps));
  else
    RUN(lafs_scale_cast_bf16(g, d->dim, c.s.gbm[wg_slot(d, layer_hi - 1)], d->dim, ps.scale(layer_hi - 1, 1), d->row2seq, d->n_tok, d->dim,
                             d->dropout_p, ps.seed(layer_hi - 1, 2), d->dropout_step, 0, stream));
  // One forked section = the tail of layer l2 and the head of layer l1 = l2 - 1 for every row range: with two crop-resolution
  // groups of full-length sequences the row ranges run beside each other (range i on stream i), forked and joined once per layer
  // -- the pattern hipGraph captures; a chain that stays forked across layers and meets the weight-gradient stream's events does
  // not.  -1 = no such part.
  auto section = [&](int l2, int l1) -> int {
    return forked(d, stream, p.n_ranges, p.n_ranges, [&](int i) {
      if (l2 >= 0) RUN(bwd_tail(ps, p.range[i], l2));
      if (l1 >= 0) RUN((cls && l1 == d->depth - 1) ? bwd_cls_chain(ps, p.range[i]) : bwd_head(ps, p.range[i], l1));
      return LAFS_OK;
    });
  };
  // the block's four weight gradients (block_wgrad) on the side stream
  auto wgrad = [&](int l) -> int {
    if (defer) return LAFS_OK;
    fork();
    RUN(block_wgrad(d, c, l, two ? d->wgrad_workgroups : 0, s2, cls && l == d->depth - 1));
    if (two) { done[l] = ev[evi++]; if (hipEventRecord(done[l], s2) != hipSuccess) ev_failed = true; }
    return LAFS_OK;
  };
  RUN(section(-1, layer_hi - 1));
  RUN(wgrad(layer_hi - 1));
  for (int l = layer_hi - 1; l >= layer_lo; --l) {
    // The section below rewrites what layer l+1's weight gradient reads on s2 -- gbm[(l-1)&1] (by layer l's LayerNorm backward:
    // gbm is produced one layer EARLY) and du / gba / dqkv of parity (l-1)&1 (by layer l-1's first part) -- so that launch has to
    // have retired (the two parity buffers cover a lag of one layer, not two)
    if (two && l + 1 < layer_hi && hipStreamWaitEvent(stream, done[l + 1], 0) != hipSuccess) ev_failed = true;
    const int l1 = (l - 1 >= layer_lo) ? l - 1 : -1;
    RUN(section(l, l1));
    if (l1 >= 0) RUN(wgrad(l1));
  }
  // LayerNorm parameter gradients of the layers just walked: the row chains' per-workgroup sums, as many as the plan says each
  // launch wrote, added in a fixed order (one launch for the whole range; every chain has joined `stream` by now)
  std::vector<lafs_ln_fold_item> items;
  for (int l = layer_hi - 1; l >= layer_lo; --l)
    for (int k = 0; k < 2; ++k) {
      const lafs_block_offsets& o = d->blocks[l];
      lafs_ln_fold_item it = {};
      for (int i = 0; i < p.n_ranges; ++i) {
        it.part[i] = c.ln_slot(l, k, i);
        it.n_parts[i] = k == 0 ? p.range[i].ln1_parts : p.range[i].ln2_parts;
      }
      if (cls && l == d->depth - 1 && k == 1) {       // LayerNorm 2 of the cls rows: one launch over n_seq rows, chain 0's slots
        for (int i = 0; i < 4; ++i) { it.part[i] = nullptr; it.n_parts[i] = 0; }
        it.part[0] = c.ln_slot(l, 1, 0); it.n_parts[0] = lafs_layernorm_bwd_parts(d->n_seq, d->dim);
      }
      it.dgamma = d->grad + (k == 0 ? o.ln1_g : o.ln2_g); it.dbeta = d->grad + (k == 0 ? o.ln1_b : o.ln2_b);
      items.push_back(it);
    }
  RUN(lafs_layernorm_bwd_fold(items.data(), (int)items.size(), d->dim, stream));
  if (two && hipStreamWaitEvent(stream, done[layer_lo], 0) != hipSuccess) ev_failed = true;      // join (s2 is in-order)
  LAFS_CHECK_ARG(!ev_failed, "a HIP event call of the weight-gradient stream protocol failed");
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_trunk_wgrad(const lafs_trunk_desc* d, void* workspace, int layer_hi, int layer_lo, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  RUN(check_desc(d));
  LAFS_CHECK_ARG(workspace && d->grad, "null buffer");
  LAFS_CHECK_ARG(d->wgrad_defer != 0, "lafs_trunk_wgrad needs a descriptor with wgrad_defer set (per-layer operand slots)");
  LAFS_CHECK_ARG(0 <= layer_lo && layer_lo < layer_hi && layer_hi <= d->depth, "bad layer range");
  const Carve c = carve(d, workspace, 1);
  for (int l = layer_hi - 1; l >= layer_lo; --l) RUN(block_wgrad(d, c, l, d->wgrad_workgroups, stream));
  return LAFS_OK;
}
