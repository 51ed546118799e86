// Forward filter / backward smoother of many short, independent chains (events: ripple or
// replay candidates, trials) in one launch each, gfx950.
//
// Reference: filter_one_step (decoder.py:151-172) scanned by filter_all_step (:174-187)
// and smooth_one_step (:200-226) scanned by smooth_all_step (:230-256), once per segment,
// each from the filters' own prior (a uniform (d, l) state pushed through one transition).
//
// MI355X design:
//   * the parallel axis is the segments: one 64-lane wave per segment walks it
//     sequentially and exactly -- no chunks, no warm-up, no boundary verification;
//   * the step arithmetic is the chunk-parallel scans' own (Fwd::step, Bwd::step_back,
//     band_conv over DPP shifts, fb_kernels.h), in their lane layout (lane l owns latents
//     lJ .. lJ+J-1, Lpad = 64 J), so a segment's outputs are those of the banded scans
//     run on that segment alone up to where those stop repairing (ScanConfig.tol);
//   * two launches: the forward stores alpha (both dynamics rows), logc and the
//     segment's f64 logZ; the backward starts from beta = 1 at the segment's last row and
//     reads alpha back (the launch boundary orders the stores before the loads);
//   * emission (and, backward, alpha) rows are prefetched PF steps ahead in a register
//     ring, as fwd_stream_piece and vit_forward do; the ring's addresses are clamped to the
//     segment's own last (backward: first) row, so no access leaves the segment's rows;
//   * workgroup b takes segment order[b] (longest first from the host): the long events
//     then do not form the tail of the launch.  No LDS, no grid barrier, no atomic.
#include "fb_kernels.h"
#include "segment_table.h"

namespace pmg {

struct SegParams {
  FBParams fb;   // emission, transition and outputs (alpha, logc, gamma, P)
  SegTable seg;  // the segments' rows (seg_off set)
  double* logz;  // (S)
};

// ring depths: one wave per segment and ~2 waves per SIMD, so the ring alone hides the
// memory latency, as deep as the registers allow (a backward row is 3 J floats): the
// relaxation kernels' choice (pf_relax_fwd / pf_relax_bwd), except the forward at J = 16,
// whose 4-deep ring spilled to scratch at WP = 32
template <int J> constexpr int seg_pf_fwd() { return J >= 16 ? 2 : (J >= 8 ? 4 : 8); }
template <int J> constexpr int seg_pf_bwd() { return J >= 16 ? 2 : (J >= 8 ? 4 : 8); }

// ---------------------------------------------------------------------------
// forward: steps t = a .. b-1 from the uniform state; alpha, logc, logz[s]
// ---------------------------------------------------------------------------
template <int J, int WP, int VEC>
__device__ __forceinline__ void seg_forward(const SegParams& sp) {
  constexpr int PF = seg_pf_fwd<J>();
  const FBParams& p = sp.fb;
  int s;
  int64_t t_a, t_b;
  __builtin_assume(sp.seg.seg_off != nullptr);   // the ragged set only: no equal-length branch here
  if (!seg_rows(sp.seg, p.T, blockIdx.x, s, t_a, t_b)) return;
  if (t_a >= t_b) {
    if (threadIdx.x == 0) sp.logz[s] = 0.0;
    return;
  }
  PMG_FB_LANE_SETUP
  (void)lane;
  const uint32_t row_bytes = (uint32_t)p.L * 4u;
  const int64_t last = t_b - 1;
  Fwd<J, WP> st;
  st.init_uniform(p, j0);
  double logz = 0.0;
  EmRaw<J> ring[PF];
  double mr[PF];
#pragma unroll
  for (int q = 0; q < PF; ++q) {
    const int64_t tl = t_a + q < last ? t_a + q : last;
    bem_load<J, VEC>(p, tl, j0, ring[q]);
    mr[q] = p.m[tl];
  }
  auto body = [&](int q, int64_t t, bool refill) {
    float e[J];
    order_after(ring[q].ph, st.q0[0]);
    em_exp<J>(p, j0, ring[q], e);
    const double mt = mr[q];
    slot_consumed<J>(e);
    if (refill) {
      const int64_t tl = t + PF < last ? t + PF : last;
      bem_load<J, VEC>(p, tl, j0, ring[q]);
      mr[q] = p.m[tl];
    }
    const float S = st.step(p, j0, invz, e);
    float* arow = p.alpha + t * 2 * (int64_t)p.L;
    float a0[J], a1[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      a0[j] = st.q0[j] * st.iS;
      a1[j] = (st.jmp * st.ep[j]) * st.iS;
    }
    bstore_row_n<J, VEC>(arow, row_bytes, j0, a0);
    bstore_row_n<J, VEC>(arow + p.L, row_bytes, j0, a1);
    const double lc = (double)__logf(S) + p.s_d * mt;
    bstore_f64_lane0(p.logc, t, lc);
    logz += lc;
  };
  int64_t tb = t_a;
  for (; tb + PF <= t_b; tb += PF) {
#pragma unroll
    for (int q = 0; q < PF; ++q) body(q, tb + q, true);
  }
#pragma unroll
  for (int q = 0; q < PF; ++q)
    if (tb + q < t_b) body(q, tb + q, false);
  if (threadIdx.x == 0) sp.logz[s] = logz;
}

template <int J, int WP>
__global__ void __launch_bounds__(64) k_segment_forward(SegParams sp) {
  if constexpr (J % 4 == 0) {
    if ((sp.fb.L & 3) == 0) {
      seg_forward<J, WP, 1>(sp);
      return;
    }
  }
  seg_forward<J, WP, 0>(sp);
}

// ---------------------------------------------------------------------------
// backward: beta = 1 at t = b-1, then t = b-1 .. a: gamma_t = alpha_t beta_t / sum,
// P_t = gamma_t[0] + gamma_t[1], beta_{t-1} = Trans(e_t beta_t)
// ---------------------------------------------------------------------------
template <int J>
struct SegRow {
  EmRaw<J> em;
  RowV<J> a0, a1;
};

template <int J, int VEC>
__device__ __forceinline__ void seg_row_load(const FBParams& p, int64_t t, int j0, SegRow<J>& r) {
  bem_load<J, VEC>(p, t, j0, r.em);
  const float* arow = p.alpha_in + t * 2 * (int64_t)p.L;
  bload_row<J, VEC>(arow, p.L, j0, r.a0);
  bload_row<J, VEC>(arow + p.L, p.L, j0, r.a1);
}

template <int J, int WP, int VEC>
__device__ __forceinline__ void seg_backward(const SegParams& sp) {
  constexpr int PF = seg_pf_bwd<J>();
  const FBParams& p = sp.fb;
  int s;
  int64_t t_a, t_b;
  __builtin_assume(sp.seg.seg_off != nullptr);   // the ragged set only: no equal-length branch here
  if (!seg_rows(sp.seg, p.T, blockIdx.x, s, t_a, t_b)) return;
  if (t_a >= t_b) return;
  PMG_FB_LANE_SETUP
  (void)lane;
  const int64_t L = p.L;
  Bwd<J, WP> st;
  st.init_ones(p, j0);
  SegRow<J> ring[PF];
#pragma unroll
  for (int q = 0; q < PF; ++q) seg_row_load<J, VEC>(p, t_b - 1 - q > t_a ? t_b - 1 - q : t_a, j0, ring[q]);
  auto body = [&](int q, int64_t t, bool refill) {
    float g0[J], g1[J], e[J], eb0[J], eb1[J], pp[J], V0, V1;
    order_after(ring[q].em.ph, st.b0[0]);
    em_exp<J>(p, j0, ring[q].em, e);
    e_beta(st, e, eb0, eb1, V0, V1);
    float G = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      g0[j] = ring[q].a0[j] * st.b0[j];
      g1[j] = ring[q].a1[j] * st.b1[j];
      G += g0[j] + g1[j];
    }
    slot_consumed<J>(g0);
    slot_consumed<J>(g1);
    slot_consumed<J>(eb0);
    if (refill) seg_row_load<J, VEC>(p, t - PF > t_a ? t - PF : t_a, j0, ring[q]);
    st.sums(eb0, V0, V1, &G);
    const float iG = rcp_nr(G);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      g0[j] *= iG;
      g1[j] *= iG;
      pp[j] = g0[j] + g1[j];
    }
    if (p.P) bstore_row<J, VEC>(p.P + t * L, p.L, j0, pp);
    if (p.gamma) {
      bstore_row<J, VEC>(p.gamma + t * 2 * L, p.L, j0, g0);
      bstore_row<J, VEC>(p.gamma + t * 2 * L + L, p.L, j0, g1);
    }
    if (t != t_a) st.template step_back<false>(p, invz, eb0, eb1, V0, V1, nullptr, nullptr);
  };
  int64_t tb = t_b - 1;
  for (; tb - (PF - 1) >= t_a; tb -= PF) {
#pragma unroll
    for (int q = 0; q < PF; ++q) body(q, tb - q, true);
  }
#pragma unroll
  for (int q = 0; q < PF; ++q)
    if (tb - q >= t_a) body(q, tb - q, false);
}

template <int J, int WP>
__global__ void __launch_bounds__(64) k_segment_backward(SegParams sp) {
  if constexpr (J % 4 == 0) {
    if ((sp.fb.L & 3) == 0) {
      seg_backward<J, WP, 1>(sp);
      return;
    }
  }
  seg_backward<J, WP, 0>(sp);
}

// ---------------------------------------------------------------------------
// host dispatch
// ---------------------------------------------------------------------------
typedef void (*seg_kernel_t)(SegParams);
static void seg_kernels(int J, int WP, seg_kernel_t* fwd, seg_kernel_t* bwd) {
  *fwd = nullptr;
  *bwd = nullptr;
#define PMG_SEG_CASE(JJ, WW)              \
  if (J == JJ && WP == WW) {              \
    *fwd = k_segment_forward<JJ, WW>;     \
    *bwd = k_segment_backward<JJ, WW>;    \
  }
  PMG_WAVE_ALL(PMG_SEG_CASE)
#undef PMG_SEG_CASE
}

}  // namespace pmg

using namespace pmg;

extern "C" {

int pmg_segment_smoother(const float* delta, const float* phi, const double* m, int64_t T,
                         const int64_t* seg_off, int32_t S, const int32_t* order,
                         const pmg_transition* tr, double likelihood_scale,
                         float* alpha, float* gamma, float* P, double* logc, double* logz,
                         void* stream) {
  PMG_REQUIRE(T > 0, "pmg_segment_smoother: T=%lld must be > 0", (long long)T);
  PMG_REQUIRE(S >= 1, "pmg_segment_smoother: S=%d segments (>= 1)", S);
  PMG_REQUIRE(delta, "pmg_segment_smoother: delta is null");
  PMG_REQUIRE(phi, "pmg_segment_smoother: phi is null");
  PMG_REQUIRE(m, "pmg_segment_smoother: m is null");
  PMG_REQUIRE(seg_off, "pmg_segment_smoother: seg_off is null");
  const int tr_rc = check_banded_tr("pmg_segment_smoother", tr, false);
  if (tr_rc == PMG_EINVAL) return tr_rc;
  PMG_REQUIRE(likelihood_scale == likelihood_scale, "pmg_segment_smoother: likelihood_scale is NaN");
  PMG_REQUIRE(alpha, "pmg_segment_smoother: alpha is null");
  PMG_REQUIRE(logc, "pmg_segment_smoother: logc is null");
  PMG_REQUIRE(logz, "pmg_segment_smoother: logz is null");
  if (tr_rc) return tr_rc;   // L > 1024
  SegParams sp;
  memset(&sp, 0, sizeof(sp));
  const int rc = fill_params(sp.fb, tr, T, 1, 0, likelihood_scale, 0.0);
  if (rc) return rc;
  FBParams& p = sp.fb;
  p.delta = delta;
  p.phi = phi;
  p.m = m;
  p.alpha = alpha;
  p.alpha_in = alpha;
  p.logc = logc;
  p.gamma = gamma;
  p.P = P;
  sp.seg.seg_off = seg_off;
  sp.seg.order = order;
  sp.seg.S = S;
  sp.logz = logz;
  seg_kernel_t kf, kb;
  seg_kernels(p.Lpad / 64, wave_WP(tr->band), &kf, &kb);
  PMG_REQUIRE(kf && kb, "pmg_segment_smoother: no kernel for J=%d band=%d", p.Lpad / 64, tr->band);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(kf, dim3(S), dim3(64), 0, st, sp);
  PMG_LAUNCH_CHECK();
  if (gamma || P) {
    hipLaunchKernelGGL(kb, dim3(S), dim3(64), 0, st, sp);
    PMG_LAUNCH_CHECK();
  }
  return PMG_OK;
}

}  // extern "C"
