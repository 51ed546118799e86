// Most likely (dynamics, latent) paths of the jump GPLVM: a max-plus forward scan with
// compact back-pointers, a streaming back-trace and an f64 path score, gfx950.  Two entry
// points share the device code, the trace and sum kernels, the workspace and the dispatch:
// pmg_viterbi_decode (R equal-length sequences stacked in time) and pmg_segment_viterbi (a
// ragged CSR of many short, independent events).  Each has its own forward instances.
//
// The recurrence is filter_one_step (decoder.py:151-172) with each logsumexp replaced
// by a max (the reference has no Viterbi of its own), over the device transition of
// pmg_transition (banded K0, exactly -inf beyond the band; K1 = 1/L):
//   a[d'][i] = max_d (delta_[d][i] + logA[d,d'])
//   v0[j]    = max_{|i-j|<=band} (a[0][i] + log g[|i-j|] + log invz[i])
//   v1       = max_i a[1][i] - log L                      (one scalar and arg-max per step)
//   delta_'[d'][j] = v_d'[j] + s*delta[t,j] + phi[t,j/32]
//
// MI355X design (the per-chain device code is in viterbi_kernels.h):
//   * the parallel axis is the chains: workgroup b looks its chain up in the chain table
//     (segment_table.h).  Equal-length: chain b is rows [b len, (b + 1) len).  Ragged:
//     chain order[b] (longest first from the host, so the long events do not form the tail
//     of the launch) with rows [a, b) read from seg_off on the device and clamped to
//     0 <= a <= b <= T.  Every address below is clamped to the chain's own rows, so a
//     chain's outputs depend on its own rows only and are the same, bit for bit, through
//     either entry point;
//   * one wave per chain, the filters' lane layout (lane l owns latents lJ .. lJ+J-1,
//     Lpad = 64 J); the band maximum takes its halo from the neighbouring lanes through
//     wave_shr:1 / wave_shl:1 DPP moves (the lanes past either end read -inf), as
//     band_conv does for sums; no LDS on the step;
//   * the f32 scores are re-centred every step by the largest a[d'][i] (one monotone
//     subtraction, so no arg-max moves): they stay within the emission's range however
//     long the chain;
//   * emission rows are prefetched PF steps ahead through the buffer-load row ring of
//     fwd_stream;
//   * back-pointers: one byte per (t, j), bits 0..6 = i - j + band of v0[j]'s maximiser,
//     bit 7 = the previous dynamics chosen by a[0][j] (indexed by the PREDECESSOR j, so
//     the back-trace reads byte [t][j] then bit 7 of byte [t][i], both in row t); one
//     int32 per t for the jump state, i | d << 16;
//   * back-trace: one wave per chain streams whole back-pointer rows, a piece of rows
//     at a time (coalesced 16-byte loads, the next piece in flight in registers while the
//     current one is walked in LDS); no dependent global load per step;
//   * score: a gather of the path's per-step increments in f64 (ll as rblk + delta, the
//     transition logs from the f32 device values; a chain's first row takes the prior
//     term), then one workgroup per chain adds them in a fixed order counted from the
//     chain's first row.  Nothing of the f32 scan enters it.
// No atomics, no grid barrier.
#include "segment_table.h"
#include "viterbi_kernels.h"

namespace pmg {

struct SegVitParams {
  VitParams v;   // emission, transition, workspace and outputs; v.T = all rows
  SegTable seg;  // the chains' rows
};

// this workgroup's chain; false: nothing to walk
__device__ __forceinline__ bool vit_chain(const SegVitParams& sp, VitChain& ch) {
  int64_t a, b;
  if (!seg_rows(sp.seg, sp.v.T, blockIdx.x, ch.id, a, b)) return false;
  ch.a = a;
  ch.len = b - a;
  return true;
}

// Two instances per (J, WP) on purpose, RAGGED = the table has seg_off: a kernel that takes
// the table's branch at run time keeps the ragged chain's len in registers through the step
// loop, which the equal-length one reads from its arguments, and measured 0.1-0.3 % slower
// per step on a single long sequence.  The trace, increment and sum kernels are not
// step-bound and branch.
template <int J, int WP, bool RAGGED>
__global__ void __launch_bounds__(64) k_viterbi_fwd(SegVitParams sp) {
  const VitParams& p = sp.v;
  VitChain ch;
  __builtin_assume((sp.seg.seg_off != nullptr) == RAGGED);
  if (!vit_chain(sp, ch) || (RAGGED && ch.len <= 0)) return;   // equal-length: len >= 1 from the entry point
  if constexpr (J % 4 == 0) {
    if ((p.L & 3) == 0) {
      vit_forward<J, WP, 1>(p, ch);
      return;
    }
  }
  vit_forward<J, WP, 0>(p, ch);
}

__global__ void __launch_bounds__(64) k_viterbi_trace(SegVitParams sp) {
  VitChain ch;
  if (!vit_chain(sp, ch) || ch.len <= 0) return;
  vit_trace(sp.v, ch);
}

// Per-step increments of log p(x, y) along the paths, f64.  Two kernels on purpose: the
// equal-length entry spreads all rows over a flat grid (one 256-thread workgroup per
// sequence would serialise a single long sequence), the ragged entry takes one workgroup
// per segment, whose first row is the segment's a.
__global__ void __launch_bounds__(256) k_viterbi_inc(SegVitParams sp) {
  const VitParams& p = sp.v;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.T) return;
  vit_increment(p, idx, idx % sp.seg.len == 0);
}
__global__ void __launch_bounds__(256) k_segment_viterbi_inc(SegVitParams sp) {
  VitChain ch;
  if (!vit_chain(sp, ch)) return;
  for (int64_t t = ch.a + threadIdx.x; t < ch.a + ch.len; t += 256) vit_increment(sp.v, t, t == ch.a);
}

// log_joint[chain] = sum of its increments: thread i adds steps i, i + 256, ... from the
// chain's first row in order, then a fixed tree over the 256 partial sums (the same order
// whatever else is in the call); 0 for a segment without rows
__global__ void __launch_bounds__(256) k_viterbi_sum(SegVitParams sp) {
  __shared__ double part[256];
  const VitParams& p = sp.v;
  VitChain ch;
  if (!vit_chain(sp, ch)) return;   // uniform over the workgroup
  const double v = vit_sum(p.inc + ch.a, ch.len, part);
  if (threadIdx.x == 0) p.log_joint[ch.id] = v;
}

// ---------------------------------------------------------------------------
// host dispatch
// ---------------------------------------------------------------------------
typedef void (*vit_kernel_t)(SegVitParams);
static vit_kernel_t vit_kernel(int J, int WP, bool ragged) {
#define PMG_VIT_CASE(JJ, WW) \
  if (J == JJ && WP == WW) return ragged ? k_viterbi_fwd<JJ, WW, true> : k_viterbi_fwd<JJ, WW, false>;
  PMG_WAVE_ALL(PMG_VIT_CASE)
#undef PMG_VIT_CASE
  return nullptr;
}

// workspace of T rows (all chains together) and S chains; returns its size in bytes
static size_t carve_vit(void* ws, int64_t T, int Lpad, int S, VitParams* p) {
  Carver c(ws);
  uint8_t* bp = c.take<uint8_t>((size_t)T * Lpad);
  int32_t* jp = c.take<int32_t>((size_t)T);
  int32_t* last = c.take<int32_t>((size_t)S * 2);
  double* inc = c.take<double>((size_t)T);
  if (p) {
    p->bp = bp;
    p->jp = jp;
    p->last = last;
    p->inc = inc;
  }
  return c.off + 256;
}

static size_t vit_workspace_size(int64_t T, int32_t L, int32_t S) {
  if (L <= 0 || pick_J(L) < 0 || T <= 0 || S < 1) return 0;
  return carve_vit(nullptr, T, 64 * pick_J(L), S, nullptr);
}

// The checks, parameters and launches both entry points share; `fn` opens the error
// texts.  T: all rows of the call; seg_off null: S sequences of len rows each (T = S len).
static int vit_decode(const char* fn, const float* delta, const float* phi, const double* rblk, int64_t T,
                      const int64_t* seg_off, int64_t len, int32_t S, const int32_t* order, const pmg_transition* tr,
                      const double* log_pi0, double likelihood_scale, int32_t* path_d, int32_t* path_l,
                      double* log_joint, void* workspace, size_t workspace_bytes, void* stream) {
  const int tr_rc = check_banded_tr(fn, tr, true);
  if (tr_rc == PMG_EINVAL) return tr_rc;
  PMG_REQUIRE(log_pi0, "%s: log_pi0 is null", fn);
  PMG_REQUIRE(likelihood_scale == likelihood_scale, "%s: likelihood_scale is NaN", fn);
  PMG_REQUIRE(path_d, "%s: path_d is null", fn);
  PMG_REQUIRE(path_l, "%s: path_l is null", fn);
  PMG_REQUIRE(log_joint, "%s: log_joint is null", fn);
  PMG_REQUIRE(workspace, "%s: workspace is null", fn);
  if (tr_rc) return tr_rc;   // L > 1024
  const size_t need = vit_workspace_size(T, tr->L, S);
  PMG_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes %zu < %zu", fn, workspace_bytes, need);
  const int64_t inc_blocks = (T + 255) / 256;   // of the equal-length entry's flat grid
  PMG_REQUIRE(seg_off || inc_blocks <= 0x7fffffffll, "%s: T * R = %lld too large", fn, (long long)T);

  const int J = pick_J(tr->L);
  SegVitParams sp;
  memset(&sp, 0, sizeof(sp));
  VitParams& p = sp.v;
  vit_fill_params(p, tr, J, likelihood_scale);
  p.delta = delta;
  p.phi = phi;
  p.rblk = rblk;
  p.log_pi0 = log_pi0;
  p.T = T;
  p.R = S;
  carve_vit(workspace, T, p.Lpad, S, &p);
  p.path_d = path_d;
  p.path_l = path_l;
  p.log_joint = log_joint;
  sp.seg.seg_off = seg_off;
  sp.seg.order = order;
  sp.seg.len = len;
  sp.seg.S = S;

  const vit_kernel_t kf = vit_kernel(J, wave_WP(tr->band), seg_off != nullptr);
  PMG_REQUIRE(kf, "%s: no kernel for J=%d band=%d", fn, J, tr->band);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(kf, dim3(S), dim3(64), 0, st, sp);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_viterbi_trace, dim3(S), dim3(64), 0, st, sp);
  PMG_LAUNCH_CHECK();
  if (seg_off)
    hipLaunchKernelGGL(k_segment_viterbi_inc, dim3(S), dim3(256), 0, st, sp);
  else
    hipLaunchKernelGGL(k_viterbi_inc, dim3((unsigned)inc_blocks), dim3(256), 0, st, sp);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_viterbi_sum, dim3(S), dim3(256), 0, st, sp);
  PMG_LAUNCH_CHECK();
  return PMG_OK;
}

}  // namespace pmg

using namespace pmg;

extern "C" {

size_t pmg_viterbi_workspace_size(int64_t T, int32_t L, int32_t R) {
  if (T <= 0 || R < 1 || R > 65535) return 0;
  return vit_workspace_size(T * R, L, R);
}

size_t pmg_segment_viterbi_workspace_size(int64_t T, int32_t L, int32_t S) { return vit_workspace_size(T, L, S); }

int pmg_viterbi_decode(const float* delta, const float* phi, const double* rblk, int64_t T, int32_t R,
                       const pmg_transition* tr, const double* log_pi0, double likelihood_scale,
                       int32_t* path_d, int32_t* path_l, double* log_joint, void* workspace,
                       size_t workspace_bytes, void* stream) {
  PMG_REQUIRE(T > 0, "pmg_viterbi_decode: T=%lld must be > 0", (long long)T);
  PMG_REQUIRE(R >= 1 && R <= 65535, "pmg_viterbi_decode: R=%d sequences (1 .. 65535)", R);
  PMG_REQUIRE(delta, "pmg_viterbi_decode: delta is null");
  PMG_REQUIRE(phi, "pmg_viterbi_decode: phi is null");
  PMG_REQUIRE(rblk, "pmg_viterbi_decode: rblk is null");
  return vit_decode("pmg_viterbi_decode", delta, phi, rblk, T * R, nullptr, T, R, nullptr, tr, log_pi0, likelihood_scale,
                    path_d, path_l, log_joint, workspace, workspace_bytes, stream);
}

int pmg_segment_viterbi(const float* delta, const float* phi, const double* rblk, int64_t T,
                        const int64_t* seg_off, int32_t S, const int32_t* order,
                        const pmg_transition* tr, const double* log_pi0, double likelihood_scale,
                        int32_t* path_d, int32_t* path_l, double* log_joint,
                        void* workspace, size_t workspace_bytes, void* stream) {
  PMG_REQUIRE(T > 0, "pmg_segment_viterbi: T=%lld must be > 0", (long long)T);
  PMG_REQUIRE(S >= 1, "pmg_segment_viterbi: S=%d segments (>= 1)", S);
  PMG_REQUIRE(delta, "pmg_segment_viterbi: delta is null");
  PMG_REQUIRE(phi, "pmg_segment_viterbi: phi is null");
  PMG_REQUIRE(rblk, "pmg_segment_viterbi: rblk is null");
  PMG_REQUIRE(seg_off, "pmg_segment_viterbi: seg_off is null");
  return vit_decode("pmg_segment_viterbi", delta, phi, rblk, T, seg_off, 0, S, order, tr, log_pi0, likelihood_scale,
                    path_d, path_l, log_joint, workspace, workspace_bytes, stream);
}

}  // extern "C"
