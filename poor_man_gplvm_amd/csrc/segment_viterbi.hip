// Most likely (dynamics, latent) paths of many short, independent chains (events: ripple
// or replay candidates, trials) in one call, gfx950: the max-plus scan, back-trace and
// f64 path score of viterbi.hip walked over a ragged CSR of segments.
//
// MI355X design:
//   * the parallel axis is the segments, as in segments.hip: workgroup b takes segment
//     order[b] (longest first from the host, so the long events do not form the tail of
//     the launch), reads its rows [a, b) from seg_off on the device and clamps them to
//     0 <= a <= b <= T;
//   * one 64-lane wave per segment runs vit_forward (viterbi_kernels.h) on the segment's
//     rows alone: the t = 0 prior, the re-centring, the tie rule and the prefetch ring are
//     the single-sequence kernel's, instruction for instruction, with the sequence base
//     r T replaced by a and the length T by b - a.  The ring's addresses are clamped to
//     the segment's last row, so no load or store addresses another segment's rows;
//   * the back-trace is vit_trace on the same rows: the piece grid starts at the
//     segment's first row and the 16-byte loads are clamped to its last 16-byte group;
//   * the score: one workgroup per segment writes the f64 increments of its rows (a row
//     is "t = 0" when it is the segment's first), a second one adds them in the order of
//     k_viterbi_sum relative to the segment's start: log_joint is that of the
//     single-sequence call on the segment alone, bit for bit.
// No LDS on the forward step, no atomics, no grid barrier; a segment's outputs depend on
// its own rows only.
#include "viterbi_kernels.h"

namespace pmg {

struct SegVitParams {
  VitParams v;             // emission, transition, workspace and outputs; v.T = all rows
  const int64_t* seg_off;  // (S + 1) row offsets
  const int32_t* order;    // (S) segment of each workgroup, or null
  int S;
};

__device__ __forceinline__ int64_t sv_uniform_i64(int64_t v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
  const int hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// this workgroup's segment and its rows [a, b), clamped to 0 <= a <= b <= T (the entry
// point cannot read the offsets); false: nothing to do
__device__ __forceinline__ bool sv_rows(const SegVitParams& sp, int& s, int64_t& a, int64_t& b) {
  const int blk = blockIdx.x;
  s = sp.order ? __builtin_amdgcn_readfirstlane(sp.order[blk]) : blk;
  if ((unsigned)s >= (unsigned)sp.S) return false;
  a = sv_uniform_i64(sp.seg_off[s]);
  b = sv_uniform_i64(sp.seg_off[s + 1]);
  const int64_t T = sp.v.T;
  a = a < 0 ? 0 : (a > T ? T : a);
  b = b < a ? a : (b > T ? T : b);
  return true;
}

template <int J, int WP>
__global__ void __launch_bounds__(64) k_segment_viterbi_fwd(SegVitParams sp) {
  const VitParams& p = sp.v;
  int s;
  int64_t a, b;
  if (!sv_rows(sp, s, a, b)) return;
  if (a >= b) {
    if (threadIdx.x == 0) p.log_joint[s] = 0.0;
    return;
  }
  const VitSeg ch = {s, a, b - a};
  if constexpr (J % 4 == 0) {
    if ((p.L & 3) == 0) {
      vit_forward<J, WP, 1>(p, ch);
      return;
    }
  }
  vit_forward<J, WP, 0>(p, ch);
}

__global__ void __launch_bounds__(64) k_segment_viterbi_trace(SegVitParams sp) {
  const VitParams& p = sp.v;
  int s;
  int64_t a, b;
  if (!sv_rows(sp, s, a, b) || a >= b) return;
  const VitSeg ch = {s, a, b - a};
  vit_trace(p, ch);
}

// per-step increments of log p(x, y) along the paths, f64: one workgroup per segment,
// the segment's first row takes the prior term
__global__ void __launch_bounds__(256) k_segment_viterbi_inc(SegVitParams sp) {
  const VitParams& p = sp.v;
  int s;
  int64_t a, b;
  if (!sv_rows(sp, s, a, b)) return;
  for (int64_t t = a + threadIdx.x; t < b; t += 256) vit_increment(p, t, t == a);
}

// log_joint[s] = sum of the segment's increments, in k_viterbi_sum's order from its start
__global__ void __launch_bounds__(256) k_segment_viterbi_sum(SegVitParams sp) {
  __shared__ double part[256];
  const VitParams& p = sp.v;
  int s;
  int64_t a, b;
  if (!sv_rows(sp, s, a, b) || a >= b) return;   // uniform over the workgroup
  const double v = vit_sum(p.inc + a, b - a, part);
  if (threadIdx.x == 0) p.log_joint[s] = v;
}

// ---------------------------------------------------------------------------
// host dispatch
// ---------------------------------------------------------------------------
typedef void (*segvit_kernel_t)(SegVitParams);
static segvit_kernel_t segvit_kernel(int J, int WP) {
#define PMG_SEGVIT_CASE(JJ, WW) \
  if (J == JJ && WP == WW) return k_segment_viterbi_fwd<JJ, WW>;
  PMG_VIT_ALL(PMG_SEGVIT_CASE)
#undef PMG_SEGVIT_CASE
  return nullptr;
}

struct SegVitWork {
  uint8_t* bp;    // [T][Lpad]
  int32_t* jp;    // [T]
  int32_t* last;  // [S][2]
  double* inc;    // [T]
};

static SegVitWork carve_segvit(void* ws, int64_t T, int Lpad, int S, size_t* total = nullptr) {
  Carver c(ws);
  SegVitWork w;
  w.bp = c.take<uint8_t>((size_t)T * Lpad);
  w.jp = c.take<int32_t>((size_t)T);
  w.last = c.take<int32_t>((size_t)S * 2);
  w.inc = c.take<double>((size_t)T);
  if (total) *total = c.off + 256;
  return w;
}

}  // namespace pmg

using namespace pmg;

extern "C" {

size_t pmg_segment_viterbi_workspace_size(int64_t T, int32_t L, int32_t S) {
  const int J = vit_J(L);
  if (J < 0 || T <= 0 || S < 1) return 0;
  size_t total = 0;
  carve_segvit(nullptr, T, 64 * J, S, &total);
  return total;
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
  PMG_REQUIRE(tr, "pmg_segment_viterbi: tr is null");
  PMG_REQUIRE(tr->L > 0 && tr->invz, "pmg_segment_viterbi: tr: bad transition (L=%d, invz %s)", tr->L,
              tr->invz ? "set" : "null");
  PMG_REQUIRE(tr->band >= 0 && tr->band <= kMaxBand && tr->band < tr->L,
              "pmg_segment_viterbi: tr: continuous-kernel band %d outside [0, min(%d, L-1)] (dense kernels: unsupported)",
              tr->band, kMaxBand);
  PMG_REQUIRE(log_pi0, "pmg_segment_viterbi: log_pi0 is null");
  PMG_REQUIRE(likelihood_scale == likelihood_scale, "pmg_segment_viterbi: likelihood_scale is NaN");
  PMG_REQUIRE(path_d, "pmg_segment_viterbi: path_d is null");
  PMG_REQUIRE(path_l, "pmg_segment_viterbi: path_l is null");
  PMG_REQUIRE(log_joint, "pmg_segment_viterbi: log_joint is null");
  PMG_REQUIRE(workspace, "pmg_segment_viterbi: workspace is null");
  const int J = vit_J(tr->L);
  if (J < 0) {
    set_error("pmg_segment_viterbi: L=%d > 1024 unsupported", tr->L);
    return PMG_EUNSUPPORTED;
  }
  const size_t need = pmg_segment_viterbi_workspace_size(T, tr->L, S);
  PMG_REQUIRE(workspace_bytes >= need, "pmg_segment_viterbi: workspace_bytes %zu < %zu", workspace_bytes, need);

  SegVitParams sp;
  memset(&sp, 0, sizeof(sp));
  VitParams& p = sp.v;
  vit_fill_params(p, tr, J, likelihood_scale);
  p.delta = delta;
  p.phi = phi;
  p.rblk = rblk;
  p.log_pi0 = log_pi0;
  p.T = T;
  p.R = 1;
  const SegVitWork w = carve_segvit(workspace, T, p.Lpad, S);
  p.bp = w.bp;
  p.jp = w.jp;
  p.last = w.last;
  p.inc = w.inc;
  p.path_d = path_d;
  p.path_l = path_l;
  p.log_joint = log_joint;
  sp.seg_off = seg_off;
  sp.order = order;
  sp.S = S;

  const segvit_kernel_t kf = segvit_kernel(J, vit_WP(tr->band));
  PMG_REQUIRE(kf, "pmg_segment_viterbi: no kernel for J=%d band=%d", J, tr->band);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(kf, dim3(S), dim3(64), 0, st, sp);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_segment_viterbi_trace, dim3(S), dim3(64), 0, st, sp);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_segment_viterbi_inc, dim3(S), dim3(256), 0, st, sp);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_segment_viterbi_sum, dim3(S), dim3(256), 0, st, sp);
  PMG_LAUNCH_CHECK();
  return PMG_OK;
}

}  // extern "C"
