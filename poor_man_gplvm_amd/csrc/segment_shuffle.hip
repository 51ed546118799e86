// Shuffle significance of many short, independent chains (events: ripple or replay
// candidates, trials), gfx950: the forward filter's log marginal of every (segment, shuffle)
// pair in one launch, each shuffle re-reading the one emission the event already has.
//
// The reference decodes once per shuffle (reactivation_analysis.py,
// circular_shuffle_spikes_within_epoch_and_decode).  The two replay shuffles served here need
// no new emission: a time-bin shuffle permutes an event's rows (perm), a column-cycle shuffle
// rotates each row along the latent axis (rot).
//
// MI355X design:
//   * one 64-lane wave per (segment, shuffle); workgroup b takes segment order[b / R] and
//     shuffle b % R (as segment_sample.hip), so the R shuffles of an event are neighbours in
//     the launch and share its emission rows in L2;
//   * the step is seg_forward's (segments.hip): Fwd::step in the scans' lane layout, the
//     emission through em_exp, lc = (double)__logf(S) + s m[src]; only the f64 sum of lc is
//     written: 8 bytes per (segment, shuffle), no alpha, logc, workspace, LDS or atomics;
//   * the register prefetch ring of seg_forward, with its row addresses taken from perm: the
//     (row, rotation) indices of a step are fetched 2 PF steps ahead (wave-uniform loads), so
//     they are there when the step's rows are requested PF steps ahead;
//   * ROT = false is the same loads and the same em_exp on another row address, so a value is
//     bit for bit what pmg_segment_smoother writes on the gathered rows;
//   * ROT = true: lane l's latent x takes the source row's latent (x + rot) mod L.  The J delta
//     values are dword buffer loads bounded to the row; the J consecutive sources wrap at most
//     once and straddle at most two phi blocks before the wrap, while after it they lie in
//     block 0 (J <= 16 < 32), so three phi loads (first block, the next, block 0) cover them;
//   * perm is clamped into the segment's [a, b) and rot is reduced into [0, L) here, so no
//     address leaves the segment's rows whatever the index arrays hold.
#include "fb_kernels.h"
#include "segment_table.h"

namespace pmg {

struct ShufParams {
  FBParams fb;          // emission and transition (no outputs)
  SegTable seg;         // the segments' rows (seg_off set), one per group of R workgroups
  const int32_t* perm;  // (R, T) source row of each step, or null: the step's own row
  const int32_t* rot;   // (R, T) latent rotation of each step, or null (ROT = false)
  double* logz;         // (R, S)
  int R;
};

template <int J> constexpr int shuf_pf() { return J >= 16 ? 2 : (J >= 8 ? 4 : 8); }

// one step's operands: ROT = false is seg_forward's slot (ph[0] alone is used)
template <int J>
struct ShufRow {
  EmRaw<J> em;
  float ph1, ph2;   // ROT: phi of the block after em.ph's and of block 0
  double m;
  int rt;           // ROT: the step's rotation in [0, L)
};

// a lane's first source latent: x0 = (j0 + rt) mod L for every lane that owns a latent < L
__device__ __forceinline__ int shuf_x0(int j0, int rt, int L) {
  const int x = j0 + rt;
  return x >= L ? x - L : x;
}

template <int J, int VEC, bool ROT>
__device__ __forceinline__ void shuf_row_load(const FBParams& p, int64_t src, int rt, int j0, ShufRow<J>& r) {
  if constexpr (!ROT) {
    bem_load<J, VEC>(p, src, j0, r.em);
  } else {
    const int x0 = shuf_x0(j0, rt, p.L);
    const __amdgpu_buffer_rsrc_t rd = rsrc_of(p.delta + src * p.ldd, (uint32_t)p.L * 4u);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      int x = x0 + j;
      x = x >= p.L ? x - p.L : x;   // lanes past L may still be >= L: the bounded load returns 0
      r.em.d.set(j, __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rd, x * 4, 0, 0)));
    }
    const __amdgpu_buffer_rsrc_t rs = rsrc_of(p.phi + src * p.ldphi, (uint32_t)p.nblk * 4u);
    const int b0 = x0 >> 5;
    r.em.ph = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, b0 * 4, 0, 0));
    r.ph1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (b0 + 1) * 4, 0, 0));
    r.ph2 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, 0, 0, 0));
    r.rt = rt;
  }
  r.m = p.m[src];
}

// em_exp's arithmetic with each latent's own block reference
template <int J>
__device__ __forceinline__ void shuf_em_exp_rot(const FBParams& p, int j0, const ShufRow<J>& r, float e[J]) {
  const int x0 = shuf_x0(j0, r.rt, p.L);
  const int b0 = x0 >> 5;
  // values, not references into the slot: a select between two fields' addresses would keep
  // the whole ring in scratch
  const float pa = r.em.ph, pb = r.ph1, pc = r.ph2;
  float a[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int x = x0 + j;
    const float ph = x >= p.L ? pc : ((x >> 5) == b0 ? pa : pb);
    a[j] = fmaf(p.s, r.em.d[j], ph);
  }
#pragma unroll
  for (int j = 0; j < J; ++j) e[j] = (j0 + j < p.L) ? exp_acc(a[j]) : 0.f;
}

template <int J, int WP, int VEC, bool ROT>
__device__ __forceinline__ void seg_shuffle(const ShufParams& sp) {
  constexpr int PF = shuf_pf<J>();
  const FBParams& p = sp.fb;
  const int blk = blockIdx.x;
  const int grp = blk / sp.R;
  const int r = blk - grp * sp.R;
  int s;
  int64_t t_a, t_b;
  __builtin_assume(sp.seg.seg_off != nullptr);   // the ragged set only: no equal-length branch here
  if (!seg_rows(sp.seg, p.T, grp, s, t_a, t_b)) return;
  double* out = sp.logz + (int64_t)r * sp.seg.S + s;
  if (t_a >= t_b) {
    if (threadIdx.x == 0) *out = 0.0;
    return;
  }
  PMG_FB_LANE_SETUP
  (void)lane;
  const int64_t last = t_b - 1;
  const int32_t* prow = sp.perm ? sp.perm + (int64_t)r * p.T : nullptr;
  const int32_t* rrow = ROT ? sp.rot + (int64_t)r * p.T : nullptr;
  // the source row (clamped into [t_a, last]) and the rotation (reduced into [0, L)) of step t
  auto idx_load = [&](int64_t t, int64_t& src, int& rt) {
    t = t < last ? t : last;
    int64_t v = prow ? (int64_t)__builtin_amdgcn_readfirstlane(prow[t]) : t;
    v = v < t_a ? t_a : v;
    src = v > last ? last : v;
    rt = 0;
    if constexpr (ROT) {
      int x = __builtin_amdgcn_readfirstlane(rrow[t]) % p.L;
      rt = x < 0 ? x + p.L : x;
    }
  };
  Fwd<J, WP> st;
  st.init_uniform(p, j0);
  double logz = 0.0;
  ShufRow<J> ring[PF];
  int64_t isrc[PF];   // slot q: the indices of the step whose rows the slot's next refill loads
  int irt[PF];
#pragma unroll
  for (int q = 0; q < PF; ++q) {
    idx_load(t_a + q, isrc[q], irt[q]);
    shuf_row_load<J, VEC, ROT>(p, isrc[q], irt[q], j0, ring[q]);
  }
#pragma unroll
  for (int q = 0; q < PF; ++q) idx_load(t_a + PF + q, isrc[q], irt[q]);
  auto body = [&](int q, int64_t t, bool refill) {
    float e[J];
    order_after(ring[q].em.ph, st.q0[0]);
    if constexpr (ROT) shuf_em_exp_rot<J>(p, j0, ring[q], e);
    else em_exp<J>(p, j0, ring[q].em, e);
    const double mt = ring[q].m;
    slot_consumed<J>(e);
    if (refill) {
      shuf_row_load<J, VEC, ROT>(p, isrc[q], irt[q], j0, ring[q]);
      idx_load(t + 2 * PF, isrc[q], irt[q]);
    }
    const float S = st.step(p, j0, invz, e);
    const double lc = (double)__logf(S) + p.s_d * mt;
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
  if (threadIdx.x == 0) *out = logz;
}

template <int J, int WP, bool ROT>
__global__ void __launch_bounds__(64) k_segment_shuffle(ShufParams sp) {
  if constexpr (J % 4 == 0 && !ROT) {   // the rotated rows are dword loads: one path
    if ((sp.fb.L & 3) == 0) {
      seg_shuffle<J, WP, 1, ROT>(sp);
      return;
    }
  }
  seg_shuffle<J, WP, 0, ROT>(sp);
}

typedef void (*shuf_kernel_t)(ShufParams);
static shuf_kernel_t shuf_kernel(int J, int WP, bool rot) {
  shuf_kernel_t k = nullptr;
#define PMG_SHUF_CASE(JJ, WW) \
  if (J == JJ && WP == WW) k = rot ? k_segment_shuffle<JJ, WW, true> : k_segment_shuffle<JJ, WW, false>;
  PMG_WAVE_ALL(PMG_SHUF_CASE)
#undef PMG_SHUF_CASE
  return k;
}

}  // namespace pmg

using namespace pmg;

extern "C" {

int pmg_segment_shuffle_logz(const float* delta, const float* phi, const double* m, int64_t T,
                             const int64_t* seg_off, int32_t S, const int32_t* order,
                             const pmg_transition* tr, double likelihood_scale,
                             const int32_t* perm, const int32_t* rot, int32_t R,
                             double* logz, void* stream) {
  PMG_REQUIRE(T > 0, "pmg_segment_shuffle_logz: T=%lld must be > 0", (long long)T);
  PMG_REQUIRE(S >= 1, "pmg_segment_shuffle_logz: S=%d segments (>= 1)", S);
  PMG_REQUIRE(R >= 1, "pmg_segment_shuffle_logz: R=%d shuffles (>= 1)", R);
  PMG_REQUIRE((int64_t)S * R <= 0x7fffffffLL, "pmg_segment_shuffle_logz: S=%d x R=%d workgroups exceed the grid", S, R);
  PMG_REQUIRE(!perm || T <= 0x7fffffffLL, "pmg_segment_shuffle_logz: T=%lld rows exceed perm's int32", (long long)T);
  PMG_REQUIRE(delta, "pmg_segment_shuffle_logz: delta is null");
  PMG_REQUIRE(phi, "pmg_segment_shuffle_logz: phi is null");
  PMG_REQUIRE(m, "pmg_segment_shuffle_logz: m is null");
  PMG_REQUIRE(seg_off, "pmg_segment_shuffle_logz: seg_off is null");
  const int tr_rc = check_banded_tr("pmg_segment_shuffle_logz", tr, false);
  if (tr_rc == PMG_EINVAL) return tr_rc;
  PMG_REQUIRE(likelihood_scale == likelihood_scale, "pmg_segment_shuffle_logz: likelihood_scale is NaN");
  PMG_REQUIRE(logz, "pmg_segment_shuffle_logz: logz is null");
  if (tr_rc) return tr_rc;   // L > 1024
  ShufParams sp;
  memset(&sp, 0, sizeof(sp));
  const int rc = fill_params(sp.fb, tr, T, 1, 0, likelihood_scale, 0.0);
  if (rc) return rc;
  FBParams& p = sp.fb;
  p.delta = delta;
  p.phi = phi;
  p.m = m;
  sp.seg.seg_off = seg_off;
  sp.seg.order = order;
  sp.seg.S = S;
  sp.perm = perm;
  sp.rot = rot;
  sp.logz = logz;
  sp.R = R;
  const shuf_kernel_t kf = shuf_kernel(p.Lpad / 64, wave_WP(tr->band), rot != nullptr);
  PMG_REQUIRE(kf, "pmg_segment_shuffle_logz: no kernel for J=%d band=%d", p.Lpad / 64, tr->band);
  hipLaunchKernelGGL(kf, dim3((unsigned)((int64_t)S * R)), dim3(64), 0, as_stream(stream), sp);
  PMG_LAUNCH_CHECK();
  return PMG_OK;
}

}  // extern "C"
