// K35: Huber-clipped additive Holt-Winters grid fit (robust_holt_winters) as a
// time-parallel scan with a SPECULATED clip pattern.
//
// The recursion (ops/smoothing.py ref_es_fit_robust, docs/BRAIN_SPEC.md): with
// the one-step error e = x - (l + t + s) and a per-row threshold c,
//     ec = e                    where |e| <= c
//        = copysign(c, e)       where |e| >  c   (the sample is pulled to pred +- c)
//     l' = l + t + a ec,   t' = t + a b ec,   s' = s + g (1 - a) ec,   loss += ec^2
// An unclipped step is hw_scan.hip's linear map v' = A v + k u (v = (l, t),
// u = x - s, k = (a, a b), A = J - k 1^T); a clipped step is v' = J v +- c k and
// a missing sample v' = J v.  The recursion is piecewise affine: WHICH piece a
// step takes depends on the state, so the plain scan does not apply.  But once
// the pattern of clipped steps (and their signs) of a lap is fixed, the lap is
// an affine scan again.  So each lap guesses the pattern, scans, runs the true
// recursion, and checks the guess:
//   pass 1  each lane folds its chunk of C steps into an affine map
//           v -> M v + b under its mask of clipped steps (all zero on a lap's
//           first attempt; lane 0 starts from the lap's entering state);
//   scan    Hillis-Steele over the 64 lanes: with a zero mask and no missing
//           sample every chunk's matrix is A^C and the lane-uniform powers
//           A^{C 2^j} from LDS serve (hw_scan.hip's scan); otherwise explicit
//           2x2 chunk matrices (J for clipped and for missing steps);
//   pass 2  the true clipped recursion over the chunk from the entering
//           state the scan delivered: tentative seasons, loss, counts and the
//           decisions the chunk really takes (one clipped bit and one sign bit
//           per step);
//   check   one ballot: every lane's decisions equal its mask -> commit the
//           tentative values; else the decisions become the masks, again.
// Lane 0 enters from the lap's state, so its decisions are final after the
// first attempt; lane i's entering state depends on the masks of lanes < i
// only, so it is final after attempt i + 1: at most 65 attempts, and a lap
// without a clipped step costs exactly one (the plain scan fit's work plus the
// compare).  After the first attempt a lap stays on the explicit-matrix scan,
// so the entering states of two attempts with the same masks are the same bits
// (the two scans round differently: a decision within rounding of c could
// otherwise flip back and forth between them).
//
// Layout: one workgroup per row, the row staged once in LDS from its first
// finite sample; one wave per candidate pair (packed fp32), up to 8 waves, the
// pairs beyond in further passes; lane i owns lap offsets [iC, iC + C) and
// keeps two register sets of C seasonal pairs (committed / tentative) for the
// whole fit, which is why a workgroup stops at 8 waves: 256 VGPRs per lane.
// Steps past a lap's end are exact no-ops (masked), for any m <= 64 C.
// The workgroup picks the winner by hw2_forecast_kernel's rule (the first
// smallest finite loss, else the last candidate); only the winning wave parks
// its seasons, and the workgroup writes forecast, sigma, state and seasons.
#include "fm_common.h"

using namespace fm;

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

struct M2 {      // [[a, b], [c, d]] for two candidates at once
  f2 a, b, c, d;
};

__device__ __forceinline__ M2 mmul(const M2& p, const M2& q) {
  return {p.a * q.a + p.b * q.c, p.a * q.b + p.b * q.d, p.c * q.a + p.d * q.c, p.c * q.b + p.d * q.d};
}

// value of lane (lane - d) & 63 (callers ignore lanes < d); d = 1 rides DPP
// wave_shr:1 with bound_ctrl (lane 0 reads 0)
__device__ __forceinline__ float up1(float v, int d) {
  if (d == 1) return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((lane_id() - d) & 63) << 2, __builtin_bit_cast(int, v)));
}
// (the halves go through named floats: a bit_cast of a vector element reads
// the vector's first element with this clang, see hw_scan.hip)
__device__ __forceinline__ f2 up(f2 v, int d) {
  const float vx = v.x, vy = v.y;
  return (f2){up1(vx, d), up1(vy, d)};
}
__device__ __forceinline__ f2 rdl(f2 v, int l) {
  const float vx = v.x, vy = v.y;
  return (f2){__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vx), l)),
              __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vy), l))};
}
__device__ __forceinline__ f2 sel(bool cx, bool cy, f2 a, f2 b) { return (f2){cx ? a.x : b.x, cy ? a.y : b.y}; }

constexpr int kLevels = 6;          // log2(64) scan levels
constexpr int kMaxG = 32;           // candidates per row
constexpr int kMaxLaps = 128;       // season laps per row
constexpr int kWaves = 8;           // waves per workgroup: 256 VGPRs for the two season sets
constexpr int kMaxAttempts = 64;    // a lap converges in at most 65 attempts (attempt <= 64)

// LDS words ahead of the winner's seasons, after the row: pw | loss | wmin |
// lap flags | winner's level, trend
constexpr int kPwWords = kWaves * kLevels * 8;
constexpr int kTailWords = kPwWords + kMaxG + kWaves + kMaxLaps + 4;

// Row layout in LDS: sample t >= base sits at xs[at(t - base)], at(r) = r +
// (r >> S); S = ctz(C) where C % 4 == 0 and m % C == 0 (chunk starts are then
// multiples of 2^S and a lane's chunk starts an odd number of words after its
// neighbour's: no bank conflicts), else 31 (no padding).
__host__ __device__ __forceinline__ int row_at(int r, int S) { return r + (r >> S); }

template <int C>
__global__ __launch_bounds__(64 * kWaves) void hw_robust_fit_kernel(
    const float* __restrict__ x, int64_t ld, int T, const float* __restrict__ cand, int G, int m, int H,
    const float* __restrict__ clip, float* __restrict__ loss, int* __restrict__ nobs, int* __restrict__ nclip,
    float* __restrict__ state, float* __restrict__ fc, float* __restrict__ sigma, int* __restrict__ best,
    int* __restrict__ nfin, float* __restrict__ season_out, int S, int npass, int* __restrict__ probe) {
  extern __shared__ float lds[];
  const int64_t row = blockIdx.x;
  const int GP = (G + 1) >> 1;
  const int Tx = (row_at(T + 64 * C, S) + 1 + 3) & ~3;
  float* xs = lds;
  f2* pw = reinterpret_cast<f2*>(lds + Tx);
  float* loss_s = lds + Tx + kPwWords;
  int* wmin = reinterpret_cast<int*>(loss_s + kMaxG);
  int* lapnan = wmin + kWaves;
  float* lbt = reinterpret_cast<float*>(lapnan + kMaxLaps);
  float* sbst = lbt + 4;                      // the winner's seasons by absolute phase [m]
  const int tid = threadIdx.x, nth = blockDim.x;
  const int lane = lane_id(), w = wave_id(), NW = nth / FM_WAVE;
  const f2 one = {1.f, 1.f}, zero = {0.f, 0.f};
  const float* xr = x + row * ld;

  // ---- stage the row from its first finite sample; flag the laps with a gap
  int fmin = T;
  for (int i = tid; i < T; i += nth)
    if (isfinite(xr[i])) { fmin = i; break; }
  fmin = wave_min(fmin);
  if (lane == 0) wmin[w] = fmin;
  for (int i = tid; i < kMaxLaps; i += nth) lapnan[i] = 0;
  __syncthreads();
  int base = T;
  for (int v = 0; v < NW; ++v) base = min(base, wmin[v]);
  base = __builtin_amdgcn_readfirstlane(base);
  for (int i = base + tid; i < T; i += nth) {
    const float v = xr[i];
    xs[row_at(i - base, S)] = v;
    if (!isfinite(v) && i >= base + m) lapnan[(i - base - m) / m] = 1;
  }
  for (int r = T - base + tid; r < T - base + 64 * C; r += nth) xs[row_at(r, S)] = __builtin_nanf("");
  __syncthreads();

  // ---- initial level / trend (every wave, the same additions): level = mean
  // of the first season, trend = (mean of the second - mean of the first) / m
  float m1 = __builtin_nanf(""), trd = 0.f;
  int c1 = 0;
  if (base < T) {
    const int e1 = min(base + m, T), e2 = min(base + 2 * m, T);
    float sa = 0.f, sb = 0.f;
    int ca = 0, cb = 0;
    for (int i = base + lane; i < e1; i += FM_WAVE) {
      const float v = xs[row_at(i - base, S)];
      const bool f = isfinite(v);
      sa += f ? v : 0.f;
      ca += f;
    }
    for (int i = e1 + lane; i < e2; i += FM_WAVE) {
      const float v = xs[row_at(i - base, S)];
      const bool f = isfinite(v);
      sb += f ? v : 0.f;
      cb += f;
    }
    sa = wave_sum(sa); sb = wave_sum(sb); ca = wave_sum(ca); cb = wave_sum(cb);
    m1 = ca > 0 ? sa / ca : 0.f;
    const float m2 = cb > 0 ? sb / cb : 0.f;
    trd = cb > 0 ? (m2 - m1) / m : 0.f;
    c1 = ca;
  }
  m1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, m1)));
  trd = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, trd)));
  c1 = __builtin_amdgcn_readfirstlane(c1);
  // a threshold that is not finite or not positive: the row runs unclipped
  float cr = clip[row];
  cr = (isfinite(cr) && cr > 0.f) ? cr : __builtin_inff();
  const f2 cpos = {cr, cr};

  const int q0 = lane * C;
  const int x0 = row_at(q0, S);               // (q0 is a multiple of 2^S: at(q0 + j) = at(q0) + j + (j >> S))
  f2 s[C], sn[C];
  int n = 0, bg = 0;
  float bs = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < npass; ++pass) {
    const int pidx = w + pass * NW;
    const bool pvalid = pidx < GP;             // an idle wave shadows the last pair
    const int pair = pvalid ? pidx : GP - 1;
    const int ga = 2 * pair, gb = 2 * pair + 1 < G ? 2 * pair + 1 : 2 * pair;
    const f2 al = {cand[3 * ga], cand[3 * gb]};
    const f2 be = {cand[3 * ga + 1], cand[3 * gb + 1]}, gm = {cand[3 * ga + 2], cand[3 * gb + 2]};
    const f2 ab = al * be, gs = gm * (one - al);
    {
      // the wave's lane-uniform powers A^{C 2^lv}, A = J - k 1^T
      const M2 A = {one - al, one - al, -ab, one - ab};
      M2 Q = A;
#pragma unroll 1
      for (int k = 1; k < C; ++k) Q = mmul(Q, A);
      if (lane == 0) {
#pragma unroll 1
        for (int lv = 0; lv < kLevels; ++lv) {
          f2* p = pw + (w * kLevels + lv) * 4;
          p[0] = Q.a; p[1] = Q.b; p[2] = Q.c; p[3] = Q.d;
          Q = mmul(Q, Q);
        }
      }
    }
    __syncthreads();                            // the powers (every wave runs every pass)
    // seasonal indices from the first season (the same for every candidate)
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const int q = q0 + j;
      const float v = (q < m && base + q < T) ? xs[x0 + j + (j >> S)] : __builtin_nanf("");
      const float si = isfinite(v) ? v - m1 : 0.f;
      s[j] = (f2){si, si};
    }
    f2 l = {m1, m1}, tr = {trd, trd};
    f2 accp = zero;                             // this lane's loss over the laps (fp32: <= C * laps terms)
    int ncx = 0, ncy = 0, attempts = 0, lap = 0;
    n = 0;
#pragma unroll 1
    for (int tl = base + m; tl < T; tl += m, ++lap) {
      const f2* pwv = pw + w * kLevels * 4;
      const int nact = min(m, T - tl);
      const int last = (nact - 1) / C;          // lane holding the lap's last step
      const int cnt = nact - q0;                // active steps of this lane (may be <= 0 or > C)
      const bool gaps = lapnan[lap] != 0;
      const float* xl = xs + row_at(tl - base + q0, S);
      unsigned mcx = 0, mcy = 0, msx = 0, msy = 0;     // speculated: clipped / negative bits per step
      unsigned dcx = 0, dcy = 0, dsx = 0, dsy = 0;     // recorded by pass 2
      f2 L = zero, Tt = zero, acc = zero;
      int nn = 0;
#pragma unroll 1
      for (int attempt = 0; attempt <= kMaxAttempts; ++attempt) {
        ++attempts;
        // after the first attempt the lap stays on the explicit-matrix scan
        const bool gen = gaps || attempt > 0;
        // ---- pass 1: the chunk as an affine map under the mask.  Only the
        // lanes before `last` feed the scan, and their chunks are full, so
        // inactive steps need no care here
        f2 bL = lane == 0 ? l : zero, bT = lane == 0 ? tr : zero;
        M2 Mm = {one, zero, zero, one};
#pragma unroll
        for (int j = 0; j < C; ++j) {
          if (j % 8 == 0 && j > 0) __builtin_amdgcn_sched_barrier(0);   // bound the loads in flight (VGPRs)
          const float xq = xl[j + (j >> S)];
          const f2 wb = bL + bT;
          f2 e = (xq - s[j]) - wb;
          if (gen) {                            // wave-uniform
            const bool fin = isfinite(xq);
            const bool cx = (mcx >> j) & 1, cy = (mcy >> j) & 1;
            const f2 sc = {(msx >> j) & 1 ? -cr : cr, (msy >> j) & 1 ? -cr : cr};
            e = sel(cx, cy, sc, e);
            e = fin ? e : zero;
            // Mm <- (J - k 1^T) Mm, k = (a, a b) on a sample that is not clipped, else 0
            const bool kx = fin && !cx, ky = fin && !cy;
            const f2 kL = sel(kx, ky, al, zero), kT = sel(kx, ky, ab, zero);
            const f2 w0 = Mm.a + Mm.c, w1 = Mm.b + Mm.d;
            Mm.a = w0 - kL * w0;
            Mm.b = w1 - kL * w1;
            Mm.c = Mm.c - kT * w0;
            Mm.d = Mm.d - kT * w1;
          }
          bL = __builtin_elementwise_fma(al, e, wb);
          bT = __builtin_elementwise_fma(ab, e, bT);
        }
        // ---- scan: the prefix of lanes 0..i is the state leaving lane i
        if (!gen) {
#pragma unroll
          for (int lv = 0; lv < kLevels; ++lv) {
            const int d = 1 << lv;
            const f2 n0 = up(bL, d), n1 = up(bT, d);
            const f2 p0 = pwv[lv * 4 + 0], p1 = pwv[lv * 4 + 1], p2 = pwv[lv * 4 + 2], p3 = pwv[lv * 4 + 3];
            if (lane >= d) {
              bL = bL + p0 * n0 + p1 * n1;
              bT = bT + p2 * n0 + p3 * n1;
            }
          }
        } else {
#pragma unroll
          for (int lv = 0; lv < kLevels; ++lv) {
            const int d = 1 << lv;
            const M2 nm = {up(Mm.a, d), up(Mm.b, d), up(Mm.c, d), up(Mm.d, d)};
            const f2 n0 = up(bL, d), n1 = up(bT, d);
            if (lane >= d) {
              bL = bL + Mm.a * n0 + Mm.b * n1;
              bT = bT + Mm.c * n0 + Mm.d * n1;
              Mm = mmul(Mm, nm);
            }
          }
        }
        // exclusive prefix: the (level, trend) entering this lane's chunk (the
        // shifts first, in uniform control flow)
        const f2 shL = up(bL, 1), shT = up(bT, 1);
        L = lane == 0 ? l : shL;
        Tt = lane == 0 ? tr : shT;
        // ---- pass 2: the true recursion; inactive steps are exact no-ops
        acc = accp;
        nn = 0;
        dcx = dcy = dsx = dsy = 0;
#pragma unroll
        for (int j = 0; j < C; ++j) {
          if (j % 8 == 0 && j > 0) __builtin_amdgcn_sched_barrier(0);
          const float xq = xl[j + (j >> S)];
          const bool act = j < cnt;
          const bool fin = act && isfinite(xq);
          const f2 lt = act ? L + Tt : L;
          const f2 e = xq - (lt + s[j]);
          const bool cx = fin && __builtin_fabsf(e.x) > cr, cy = fin && __builtin_fabsf(e.y) > cr;
          const bool gx = e.x < 0.f, gy = e.y < 0.f;
          f2 ec = sel(cx, cy, sel(gx, gy, -cpos, cpos), e);
          ec = fin ? ec : zero;
          L = __builtin_elementwise_fma(al, ec, lt);
          Tt = __builtin_elementwise_fma(ab, ec, Tt);
          sn[j] = __builtin_elementwise_fma(gs, ec, s[j]);
          acc = __builtin_elementwise_fma(ec, ec, acc);
          nn += fin ? 1 : 0;
          dcx |= cx ? 1u << j : 0u;
          dcy |= cy ? 1u << j : 0u;
          dsx |= cx && gx ? 1u << j : 0u;
          dsy |= cy && gy ? 1u << j : 0u;
        }
        // ---- check: the decisions taken are the decisions assumed
        if (__all(dcx == mcx && dcy == mcy && dsx == msx && dsy == msy)) break;
        mcx = dcx; mcy = dcy; msx = dsx; msy = dsy;
      }
      // commit the lap
#pragma unroll
      for (int j = 0; j < C; ++j) s[j] = sn[j];
      accp = acc;
      n += nn;
      ncx += __builtin_popcount(dcx);
      ncy += __builtin_popcount(dcy);
      l = rdl(L, last);
      tr = rdl(Tt, last);
    }
    const float fa = wave_sum(accp.x), fb = wave_sum(accp.y);
    n = __builtin_amdgcn_readfirstlane(wave_sum(n));      // the same for every candidate
    ncx = wave_sum(ncx);
    ncy = wave_sum(ncy);

    // ---- per-candidate results
    if (lane == 0 && pvalid) {
      const int64_t pa = row * G + ga;
      loss[pa] = fa;
      nobs[pa] = n;
      nclip[pa] = ncx;
      loss_s[ga] = fa;
      if (2 * pair + 1 < G) {
        loss[pa + 1] = fb;
        nobs[pa + 1] = n;
        nclip[pa + 1] = ncy;
        loss_s[gb] = fb;
      }
      if (probe != nullptr) {                   // fm_hw_robust_set_probe: attempts, laps per pair
        probe[(row * (kMaxG / 2) + pair) * 2] = attempts;
        probe[(row * (kMaxG / 2) + pair) * 2 + 1] = lap;
      }
    }
    __syncthreads();
    // ---- the best candidate over [0, g1): the first smallest finite loss,
    // else the last candidate (one lane per candidate); a new winner parks its
    // seasons by absolute phase and its (level, trend)
    const int g0 = 2 * pass * NW, g1 = min(G, 2 * (pass + 1) * NW);
    {
      const float inf = __builtin_inff();
      const float v = lane < g1 ? loss_s[lane] : inf;
      const bool fv = lane < g1 && isfinite(v);
      const float mn = wave_min(fv ? v : inf);
      const uint64_t at_min = __ballot(fv && v == mn);
      if (at_min != 0) {
        bg = (int)__builtin_ctzll(at_min);
        bs = mn;
      } else {
        bg = g1 - 1;
        bs = loss_s[g1 - 1];
      }
      bs = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, bs)));
      bg = __builtin_amdgcn_readfirstlane(bg);
    }
    if (bg >= g0 && (bg >> 1) == pair && pvalid) {
      const bool hi = (bg & 1) != 0;
      int p = (base + q0) % m;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        if (q0 + j < m) sbst[p] = hi ? s[j].y : s[j].x;
        p = p + 1 == m ? 0 : p + 1;
      }
      if (lane == 0) {
        lbt[0] = hi ? l.y : l.x;
        lbt[1] = hi ? tr.y : tr.x;
      }
    }
  }
  __syncthreads();
  // ---- the winner's forecast, state and seasons, spread over the workgroup
  const float lb = lbt[0], tb = lbt[1];
  const int t0 = T % m;
  float* fcr = fc + row * H;
  for (int h = 1 + tid; h <= H; h += nth) {
    int p = t0 + h - 1;
    while (p >= m) p -= m;
    fcr[h - 1] = lb + h * tb + sbst[p];
  }
  if (season_out != nullptr) {
    float* so = season_out + row * m;
    for (int p = tid; p < m; p += nth) so[p] = sbst[p];
  }
  if (tid == 0) {
    sigma[row] = n > 1 ? sqrtf(bs / (float)(n - 1)) : 0.f;
    best[row] = bg;
    state[row * 3 + 0] = lb;
    state[row * 3 + 1] = tb;
    state[row * 3 + 2] = (float)t0;
    nfin[row] = c1 + n;
  }
}

constexpr int kChunks[] = {3, 4, 6, 8, 12, 16, 20, 24};
constexpr size_t kMaxLds = 160 * 1024;   // a single gfx950 workgroup may take the whole LDS

// The plan of a robust fit for (T, G, m): chunk length C (0: not covered),
// the row padding shift, waves, candidate passes and dynamic LDS bytes.  One
// place decides for the launcher and for fm_hw_robust_supported.
struct RobustPlan {
  int C = 0, S = 31, waves = 0, npass = 0;
  size_t lds = 0;
};

RobustPlan robust_plan(int T, int G, int m) {
  RobustPlan p;
  if (G < 1 || G > kMaxG || m < 3 * 64 || m > 64 * 24 || T < 2 * (int64_t)m) return p;
  if ((T - m) / m >= kMaxLaps) return p;
  const int need = (m + 63) / 64;
  int C = 0;
  for (int c : kChunks)
    if (c >= need) { C = c; break; }
  const int S = (m % C == 0 && C % 4 == 0) ? __builtin_ctz(C) : 31;
  const size_t words = ((size_t)row_at(T + 64 * C, S) + 1 + 3) & ~(size_t)3;
  const size_t lds = (words + kTailWords + (size_t)((m + 3) & ~3)) * 4;
  if (lds > kMaxLds) return p;
  const int GP = (G + 1) / 2;
  p.C = C;
  p.S = S;
  p.npass = (GP + kWaves - 1) / kWaves;
  p.waves = (GP + p.npass - 1) / p.npass;
  p.lds = lds;
  return p;
}

int* g_probe = nullptr;                  // fm_hw_robust_set_probe: [R, 16, 2] int32, or null

template <int C>
int launch(const float* x, int64_t ld, int T, int64_t R, const float* cand, int G, int m, int H, const float* clip,
           float* loss, int* nobs, int* nclip, float* state, float* fc, float* sigma, int* best, int* nfin,
           float* season_out, const RobustPlan& pl, hipStream_t stream) {
  if (pl.lds > 65536) {
    static bool done = false;            // once per instantiation (idempotent if raced)
    if (!done) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(hw_robust_fit_kernel<C>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
      done = true;
    }
  }
  hipLaunchKernelGGL((hw_robust_fit_kernel<C>), dim3((unsigned)R), dim3(64 * pl.waves), pl.lds, stream, x, ld, T, cand,
                     G, m, H, clip, loss, nobs, nclip, state, fc, sigma, best, nfin, season_out, pl.S, pl.npass,
                     g_probe);
  FM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// Attempt counters of the next fits (benchmarks/bench_hw_robust.py): int32
// [R, 16 pairs, 2] = (attempts, laps) per candidate pair, null to switch off.
FM_API int fm_hw_robust_set_probe(void* p) {
  g_probe = static_cast<int*>(p);
  return 0;
}

// 1 when fm_hw_robust_fit covers (T, G, m): 192 <= m <= 1536, G <= 32,
// 2 m <= T, fewer than 128 laps and the row within a workgroup's LDS.
FM_API int fm_hw_robust_supported(int T, int G, int m) { return robust_plan(T, G, m).C != 0; }

// Huber-clipped additive Holt-Winters grid fit + the best candidate's forecast
// in one launch (one workgroup per row).  clip [R]: the row's threshold (not
// finite or <= 0: unclipped).  Per (row, candidate): loss [R, G] (the
// truncated squared error), nobs, nclip [R, G] int32.  Per row: fc [R, H],
// sigma, best, nfin [R], the winner's state [R, 3] = (level, trend, next
// phase) and, when season_out is not null, its seasons [R, m] by absolute
// phase.  hipErrorInvalidValue for a shape fm_hw_robust_supported refuses.
FM_API int fm_hw_robust_fit(const float* x, int64_t ld, int T, int64_t R, const float* cand, int G, int m, int H,
                            const float* clip, float* loss, int* nobs, int* nclip, float* state, float* fc,
                            float* sigma, int* best, int* nfin, float* season_out, hipStream_t stream) {
  if (R <= 0) return 0;
  if (H < 0) return (int)hipErrorInvalidValue;
  const RobustPlan pl = robust_plan(T, G, m);
  if (pl.C == 0) return (int)hipErrorInvalidValue;
#define FM_HWR(CC)                                                                                                  \
  case CC:                                                                                                         \
    return launch<CC>(x, ld, T, R, cand, G, m, H, clip, loss, nobs, nclip, state, fc, sigma, best, nfin, season_out, \
                      pl, stream);
  switch (pl.C) {
    FM_HWR(3) FM_HWR(4) FM_HWR(6) FM_HWR(8) FM_HWR(12) FM_HWR(16) FM_HWR(20) FM_HWR(24)
    default: return (int)hipErrorInvalidValue;
  }
#undef FM_HWR
}
