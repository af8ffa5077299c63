// Downstream-consumer kernels: the per-step state update of the SDE sampler the reference's sample_50k.py runs
// (diffusion/transport/integrators.py:27-35 Euler-Maruyama step with the velocity -> score conversion of path.py:74-89 and the drift of
// transport.py:254-257 folded in) and the image -> uint8 conversion of sample_50k.py:151.  Both are single HBM passes.
//
// Arithmetic follows the reference's f32 elementwise graph operation by operation (no contraction into FMAs, IEEE divide), so for the same
// model output the state after a step is bit-identical to the PyTorch-CPU result; every coefficient depends on t only and arrives as a scalar
// the host computed in f32 the way the reference does.
//
// The adaptive dopri5 ODE sampler (transport.py:356-407 -> torchdiffeq.odeint, integrators.py:79-118) adds three HBM passes per solver step: the
// Runge-Kutta combine y0 + sum_j c_j k_j (stage inputs, y_mid), the error ratio (err, its tolerance-scaled mean square, partial sums per workgroup
// summed in a fixed order in f64) and the quartic dense output.  Their coefficients and k pointers travel by value in struct dmvae_ode_terms.
// The likelihood sampler adds one pass per model evaluation (dmvae_ode_hutchinson_pack): the negated velocity into the flat stage buffer and the
// per-sample Hutchinson sum of the input-VJP against the Rademacher probe.
// Classifier-free guidance (lightningdit.py:423-447) adds one pass per guided model evaluation (dmvae_cfg_combine): the model's output for the batch
// [cond | uncond] becomes what forward_with_cfg returns, with the reference's rounding sites and the interval gate read from t on the device.
// The Heun step of the SDE sampler (integrators.py:37-48) is three passes around its two model evaluations -- perturb, predict (K1 and the predictor state),
// correct --, and the "Tweedie" / "Euler" last steps (transport.py:279-288) one pass with a mode argument; autoguidance (lightningdit.py:450-465) is one pass
// over the two models' outputs (dmvae_autoguidance_combine), its interval gate read from t on the device like the guidance kernel's.
// Every pass takes any n: float4 / bf16x4 quads while all pointers allow it, then a scalar tail (quads_then_tail; ode_quads decides, launch launches).
// A noise- or score-predicting model (transport.py:171-181) adds a prologue to every model-consuming pass -- the `_m` entry points, which launch the <true>
// instantiation of the velocity ones' kernels --: v = (c0 * x) + dv * (m / nsig) or (c0 * x) + dv * m, its three t-only coefficients host scalars in
// struct dmvae_model_terms, passed by value.  dmvae_model_velocity writes v alone (the ODE samplers' drift).
#include <initializer_list>
#include <type_traits>

#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_sampler {
#pragma clang fp contract(off)

// The loop of every pass: block-256 grid-stride over the nq quads -- f(width 4, first element) --, then over the scalar tail [4 nq, n) -- f(width 1, element).
// The width arrives as a type, so f (a generic lambda) hands it on as a template argument.
template <class F>
__device__ __forceinline__ void quads_then_tail(size_t n, size_t nq, F f) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t i = tid; i < nq; i += stride) f(std::integral_constant<int, 4>{}, 4 * i);
  for (size_t e = 4 * nq + tid; e < n; e += stride) f(std::integral_constant<int, 1>{}, e);
}

// The prologue scalars of a noise / score model as a kernel argument: by value when M, an empty stand-in (last in the list: no bytes in the argument segment) otherwise
struct no_terms {};
template <bool M> using terms_arg = std::conditional_t<M, dmvae_model_terms, no_terms>;

template <int W>
__device__ __forceinline__ void load_w(const void* p, bool is_bf16, size_t e, float (&o)[W]) {
  if constexpr (W == 4) {
    if (is_bf16) {
      const bf16x4 t = *reinterpret_cast<const bf16x4*>((const bf16*)p + e);
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] = (float)t[j];
    } else {
      const float4 t = *reinterpret_cast<const float4*>((const float*)p + e);
      o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    }
  } else {
    o[0] = is_bf16 ? (float)((const bf16*)p)[e] : ((const float*)p)[e];
  }
}

template <int W>
__device__ __forceinline__ void store_w(float* p, size_t e, const float (&v)[W]) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  else p[e] = v[0];
}

template <int W>
__device__ __forceinline__ void store_w(bf16* p, size_t e, const float (&v)[W]) {      // the guidance kernels': every value is a bf16 already, the conversion exact
  if constexpr (W == 4) {
    bf16x4 t;
#pragma unroll
    for (int j = 0; j < 4; j++) t[j] = (bf16)v[j];
    *reinterpret_cast<bf16x4*>(p + e) = t;
  } else {
    p[e] = (bf16)v[0];
  }
}

// sde_drift at (y, v): v + diff * ((rar * v - y) / var)   (transport.py:253-256 over get_score_from_velocity, path.py:74-89)
__device__ __forceinline__ float sde_drift_one(float v, float y, float rar, float var, float diff) {
  const float score = (rar * v - y) / var;
  return v + diff * score;
}

// Transport.get_score of a noise / score model (transport.py:202-216): m / -sigma_t, or m itself
__device__ __forceinline__ float model_score_one(const dmvae_model_terms& P, float m) {
  return P.kind == DMVAE_MODEL_NOISE ? m / P.nsig : m;
}

// Transport.get_drift of a noise / score model at the state y (transport.py:171-181): (-drift_mean) + drift_var * score, with -drift_mean = c0 * y
__device__ __forceinline__ float model_velocity_one(const dmvae_model_terms& P, float m, float y) {
  const float a = P.c0 * y;
  const float b = P.dv * model_score_one(P, m);
  return a + b;
}

// The model's output as the velocity: itself (M false: a velocity model), or through the prologue
template <bool M>
__device__ __forceinline__ float velocity_of(const terms_arg<M>& P, float m, float y) {
  if constexpr (M) return model_velocity_one(P, m, y);
  else return m;
}

// The Euler-Maruyama step: mean = x + sde_drift * dt, x' = mean + sqrt(2 diffusion) * (w sqrt(dt)); w NULL: x_out = mean (the "Mean" last step).
// M: v is a noise / score model's output, converted at x first
template <int W, bool M>
__device__ __forceinline__ void euler_at(const float* __restrict__ x, const void* v, int v_bf16, const float* __restrict__ w, float* __restrict__ x_out,
                                         float* __restrict__ mean_out, size_t e, float rar, float var, float diff, float dt, float sq2d, float sqdt,
                                         const terms_arg<M>& P) {
  float y[W], vv[W], wv[W], mo[W], xo[W];
  load_w<W>(x, false, e, y);
  load_w<W>(v, v_bf16, e, vv);
  if (w) load_w<W>(w, false, e, wv);
#pragma unroll
  for (int j = 0; j < W; j++) {
    if (!w) wv[j] = 0.f;
    const float drift = sde_drift_one(velocity_of<M>(P, vv[j], y[j]), y[j], rar, var, diff);
    mo[j] = y[j] + drift * dt;
    xo[j] = mo[j] + sq2d * (wv[j] * sqdt);
  }
  if (mean_out) store_w<W>(mean_out, e, mo);
  if (x_out) store_w<W>(x_out, e, w ? xo : mo);
}

template <bool M>
__global__ __launch_bounds__(256) void sde_euler_kernel(const float* __restrict__ x, const void* v, int v_bf16, const float* __restrict__ w, float* __restrict__ x_out,
                                                        float* __restrict__ mean_out, size_t n, size_t nq, float rar, float var, float diff, float dt, float sq2d,
                                                        float sqdt, terms_arg<M> P) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { euler_at<W, M>(x, v, v_bf16, w, x_out, mean_out, e, rar, var, diff, dt, sq2d, sqdt, P); });
}

// y [npix][c_stride] f32 (NHWC, first c channels used) -> out [npix][c] uint8 = trunc(clamp(127.5 * s + 128, 0, 255)); s optionally rounded
// to bf16 first (what `.float()` of an autocast decoder output holds).  NaN -> 0 is not defined by the reference (float -> uint8 of NaN); here 0.
__global__ __launch_bounds__(256) void image_to_u8_kernel(const float* __restrict__ y, uint8_t* __restrict__ out, size_t npix, int c, int c_stride,
                                                          int round_bf16) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    for (int j = 0; j < c; j++) {
      float s = y[p * c_stride + j];
      if (round_bf16) s = (float)(bf16)s;
      float q = 127.5f * s + 128.0f;
      q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);            // NaN compares false twice and converts to 0 below
      out[p * c + j] = (uint8_t)(int)(q == q ? q : 0.f);
    }
  }
}


// ---- dopri5 (torchdiffeq's RKAdaptiveStepsizeODESolver; integrators.py:79-118) -------------------------------------------------------------

// s = sum_{j < nk} c_j k_j, j ascending, products and sums rounded to f32 one by one.  round_bf16: the autocast matmul of torchdiffeq's
// k.matmul(coef * dt) -- c_j and k_j rounded to bf16 (their products are exact in f32), the f32 sum rounded to bf16 at the end.
template <int W>
__device__ __forceinline__ void rk_sum(const dmvae_ode_terms& T, int round_bf16, size_t e, float (&s)[W]) {
#pragma unroll
  for (int j = 0; j < DMVAE_ODE_MAX_TERMS; j++) {             // unrolled: constant indices into the by-value struct (no scratch copy)
    if (j >= T.nk) break;
    float kv[W];
    load_w<W>(T.k[j], (T.k_bf16 >> j) & 1, e, kv);
    const float c = round_bf16 ? (float)(bf16)T.c[j] : T.c[j];
#pragma unroll
    for (int w = 0; w < W; w++) {
      const float p = c * (round_bf16 ? (float)(bf16)kv[w] : kv[w]);
      s[w] = j == 0 ? p : s[w] + p;
    }
  }
  if (round_bf16) {
#pragma unroll
    for (int w = 0; w < W; w++) s[w] = (float)(bf16)s[w];
  }
}

template <int W>
__device__ __forceinline__ void rk_combine_at(const float* __restrict__ y0, const dmvae_ode_terms& T, float* __restrict__ out, size_t e, int round_bf16) {
  float s[W];
  rk_sum<W>(T, round_bf16, e, s);
  if (y0) {
    float a[W];
    load_w<W>(y0, false, e, a);
#pragma unroll
    for (int w = 0; w < W; w++) s[w] = a[w] + s[w];
  }
  store_w<W>(out, e, s);
}

__global__ __launch_bounds__(256) void ode_rk_combine_kernel(const float* __restrict__ y0, dmvae_ode_terms T, float* __restrict__ out, size_t n, size_t nq,
                                                             int round_bf16) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { rk_combine_at<W>(y0, T, out, e, round_bf16); });
}

// err = rk_sum(c_err dt);  e = err / (atol + rtol * max(|y0|, |y1|))  (torch.max: a NaN operand gives NaN);  acc += e^2 in f64;  bad |= !isfinite(y1)
template <int W>
__device__ __forceinline__ void err_at(const float* __restrict__ y0, const float* __restrict__ y1, const dmvae_ode_terms& T, float* __restrict__ err_out,
                                       size_t e, float atol, float rtol, int round_bf16, double& acc, int& bad) {
  float s[W], a[W], b[W];
  rk_sum<W>(T, round_bf16, e, s);
  load_w<W>(y0, false, e, a);
  load_w<W>(y1, false, e, b);
#pragma unroll
  for (int w = 0; w < W; w++) {
    const float fa = fabsf(a[w]), fb = fabsf(b[w]);
    const float m = (fa > fb || fa != fa) ? fa : fb;
    const float q = s[w] / (atol + rtol * m);
    acc += (double)q * (double)q;
    bad |= !isfinite(b[w]);
  }
  if (err_out) store_w<W>(err_out, e, s);
}

__device__ __forceinline__ void block_sum_flag_256(double& v, int& f) {   // f64 sum and OR of a flag over 256 threads, both in place
  __shared__ double sv[256];
  __shared__ int sf[256];
  sv[threadIdx.x] = v;
  sf[threadIdx.x] = f;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {                       // fixed tree: the same bits on every run
    if ((int)threadIdx.x < h) { sv[threadIdx.x] = sv[threadIdx.x] + sv[threadIdx.x + h]; sf[threadIdx.x] |= sf[threadIdx.x + h]; }
    __syncthreads();
  }
  v = sv[0];
  f = sf[0];
}

__global__ __launch_bounds__(256) void ode_err_partial_kernel(const float* __restrict__ y0, const float* __restrict__ y1, dmvae_ode_terms T,
                                                              float* __restrict__ err_out, double* __restrict__ part, int* __restrict__ part_bad, size_t n,
                                                              size_t nq, float atol, float rtol, int round_bf16) {
  double acc = 0.0;
  int bad = 0;
  quads_then_tail(n, nq, [&](auto W, size_t e) { err_at<W>(y0, y1, T, err_out, e, atol, rtol, round_bf16, acc, bad); });
  block_sum_flag_256(acc, bad);
  if (threadIdx.x == 0) { part[blockIdx.x] = acc; part_bad[blockIdx.x] = bad; }
}

// one workgroup: result = {(float)(sum / n), any non-finite y1}; partials in a fixed order (strided per thread, then the fixed tree)
__global__ __launch_bounds__(256) void ode_err_final_kernel(const double* __restrict__ part, const int* __restrict__ part_bad, int nparts, size_t n,
                                                            void* __restrict__ result) {
  double acc = 0.0;
  int bad = 0;
  for (int b = threadIdx.x; b < nparts; b += 256) { acc += part[b]; bad |= part_bad[b]; }
  block_sum_flag_256(acc, bad);
  if (threadIdx.x == 0) {
    reinterpret_cast<float*>(result)[0] = (float)(acc / (double)n);
    reinterpret_cast<int*>(result)[1] = bad;
  }
}

// torchdiffeq's _interp_fit (dopri5's y_mid given) + _interp_evaluate at x, in their operation order
template <int W>
__device__ __forceinline__ void dense_at(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ ym, const void* f0, const void* f1,
                                         int f_bf16, float dt, float x, float* __restrict__ out, size_t e) {
  float Y0[W], Y1[W], YM[W], F0[W], F1[W], o[W];
  load_w<W>(y0, false, e, Y0);
  load_w<W>(y1, false, e, Y1);
  load_w<W>(ym, false, e, YM);
  load_w<W>(f0, f_bf16 & 1, e, F0);
  load_w<W>(f1, (f_bf16 >> 1) & 1, e, F1);
  const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
#pragma unroll
  for (int w = 0; w < W; w++) {
    const float a = ((2.f * dt) * (F1[w] - F0[w]) - 8.f * (Y1[w] + Y0[w])) + 16.f * YM[w];
    const float b = ((dt * (5.f * F0[w] - 3.f * F1[w]) + 18.f * Y0[w]) + 14.f * Y1[w]) - 32.f * YM[w];
    const float c = ((dt * (F1[w] - 4.f * F0[w]) - 11.f * Y0[w]) - 5.f * Y1[w]) + 16.f * YM[w];
    const float d = dt * F0[w];
    float t = Y0[w] + x * d;
    t = t + x2 * c;
    t = t + x3 * b;
    o[w] = t + x4 * a;
  }
  store_w<W>(out, e, o);
}

__global__ __launch_bounds__(256) void ode_dense_kernel(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ ym, const void* f0,
                                                        const void* f1, int f_bf16, float dt, float x, float* __restrict__ out, size_t n, size_t nq) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { dense_at<W>(y0, y1, ym, f0, f1, f_bf16, dt, x, out, e); });
}

// The likelihood sampler's stage value (transport.py:402-459, Hutchinson's trace estimator): k_x = -v (exact in f32), k_logp[b] = sum_i g[b][i] * eps[b][i].
// One workgroup per sample; eps is +-1, so every product is exact and the f64 sum -- per-thread strided partials, then a fixed tree -- is the same on every run.
template <int W>
__device__ __forceinline__ void pack_at(const void* v, int v_bf16, const float* __restrict__ g, const float* __restrict__ eps, float* __restrict__ kx, size_t e,
                                        double& acc) {
  float a[W], gv[W], ev[W], o[W];
  load_w<W>(v, v_bf16, e, a);
  load_w<W>(g, false, e, gv);
  load_w<W>(eps, false, e, ev);
#pragma unroll
  for (int w = 0; w < W; w++) {
    o[w] = -a[w];
    acc += (double)gv[w] * (double)ev[w];
  }
  store_w<W>(kx, e, o);
}

// Its own loop: 1024 threads stride over one sample, not a grid over the array (quads_then_tail's indexing)
__global__ __launch_bounds__(1024) void ode_hutchinson_pack_kernel(const void* v, int v_bf16, const float* __restrict__ g, const float* __restrict__ eps,
                                                                   float* __restrict__ kx, float* __restrict__ klogp, size_t per, int quads) {
  __shared__ double red[1024];
  const size_t base = (size_t)blockIdx.x * per;
  const size_t nq = quads ? per / 4 : 0;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < nq; i += 1024) pack_at<4>(v, v_bf16, g, eps, kx, base + 4 * i, acc);
  for (size_t e = 4 * nq + threadIdx.x; e < per; e += 1024) pack_at<1>(v, v_bf16, g, eps, kx, base + e, acc);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {                      // fixed tree
    if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) klogp[blockIdx.x] = (float)red[0];
}

// ---- classifier-free guidance (LightningDiT.forward_with_cfg, lightningdit.py:423-447) -----------------------------------------------------------

// The reference's three ATen ops on one element: d = cond - uncond, m = scale * d, g = uncond + m.  Each computes in f32; a bf16 tensor rounds (RNE) after
// every op, an f32 tensor keeps the three f32 roundings (no FMA).  gate: t[0] < cfg_interval_start -> the conditional value itself.
template <typename T>
__device__ __forceinline__ float cfg_one(float c, float u, float scale, bool gate) {
  if (gate) return c;
  if constexpr (sizeof(T) == 2) {
    const float d = (float)(bf16)(c - u);
    const float m = (float)(bf16)(scale * d);
    return (float)(bf16)(u + m);
  } else {
    const float d = c - u;
    const float m = scale * d;
    return u + m;
  }
}

// src / dst [2][half] with half = n * channels * hw elements ([2n, C, H, W] contiguous): element e of the first half is the conditional sample's, e + half the
// unconditional one's.  Channels below k: both halves receive the guided value; the others are copied.  W == 4: hw % 4 == 0, a quad never straddles a channel.
template <typename T, int W>
__device__ __forceinline__ void cfg_at(const T* __restrict__ src, T* __restrict__ dst, size_t e, size_t half, size_t hw, int channels, int k, float scale, bool gate) {
  float c[W], u[W];
  load_w<W>(src, sizeof(T) == 2, e, c);
  load_w<W>(src + half, sizeof(T) == 2, e, u);
  if ((int)((e / hw) % (size_t)channels) < k) {
#pragma unroll
    for (int j = 0; j < W; j++) c[j] = u[j] = cfg_one<T>(c[j], u[j], scale, gate);
  }
  store_w<W>(dst, e, c);
  store_w<W>(dst + half, e, u);
}

template <typename T>
__global__ __launch_bounds__(256) void cfg_combine_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t half, size_t nq, size_t hw, int channels, int k,
                                                          float scale, const float* __restrict__ t, float interval_start) {
  const bool gate = t != nullptr && t[0] < interval_start;
  quads_then_tail(half, nq, [&](auto W, size_t e) { cfg_at<T, W>(src, dst, e, half, hw, channels, k, scale, gate); });
}

// ---- Heun step of the SDE sampler (integrators.py:37-48) and the "Tweedie" / "Euler" last steps (transport.py:279-288) ------------------------------------

// xhat = x + sqrt(2 diffusion) * (w sqrt(dt))
template <int W>
__device__ __forceinline__ void heun_perturb_at(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ xhat, size_t e, float sq2d, float sqdt) {
  float a[W], b[W], o[W];
  load_w<W>(x, false, e, a);
  load_w<W>(w, false, e, b);
#pragma unroll
  for (int j = 0; j < W; j++) o[j] = a[j] + sq2d * (b[j] * sqdt);
  store_w<W>(xhat, e, o);
}

__global__ __launch_bounds__(256) void sde_heun_perturb_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ xhat, size_t n, size_t nq,
                                                               float sq2d, float sqdt) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { heun_perturb_at<W>(x, w, xhat, e, sq2d, sqdt); });
}

// K1 = sde_drift(xhat, v1);  xp = xhat + dt * K1.  M: v1 is a noise / score model's output, converted at xhat first
template <int W, bool M>
__device__ __forceinline__ void heun_predict_at(const float* __restrict__ xhat, const void* v, int v_bf16, float* __restrict__ k1, float* __restrict__ xp, size_t e,
                                                float rar, float var, float diff, float dt, const terms_arg<M>& P) {
  float y[W], vv[W], k[W], o[W];
  load_w<W>(xhat, false, e, y);
  load_w<W>(v, v_bf16, e, vv);
#pragma unroll
  for (int j = 0; j < W; j++) {
    k[j] = sde_drift_one(velocity_of<M>(P, vv[j], y[j]), y[j], rar, var, diff);
    o[j] = y[j] + dt * k[j];
  }
  store_w<W>(k1, e, k);
  store_w<W>(xp, e, o);
}

template <bool M>
__global__ __launch_bounds__(256) void sde_heun_predict_kernel(const float* __restrict__ xhat, const void* v, int v_bf16, float* __restrict__ k1, float* __restrict__ xp,
                                                               size_t n, size_t nq, float rar, float var, float diff, float dt, terms_arg<M> P) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { heun_predict_at<W, M>(xhat, v, v_bf16, k1, xp, e, rar, var, diff, dt, P); });
}

// K2 = sde_drift(xp, v2) with the coefficients at t + dt;  x = xhat + (0.5 dt) * (K1 + K2)
template <int W, bool M>
__device__ __forceinline__ void heun_correct_at(const float* __restrict__ xhat, const float* __restrict__ xp, const float* __restrict__ k1, const void* v, int v_bf16,
                                                float* __restrict__ out, size_t e, float rar, float var, float diff, float hdt, const terms_arg<M>& P) {
  float y[W], p[W], k[W], vv[W], o[W];
  load_w<W>(xhat, false, e, y);
  load_w<W>(xp, false, e, p);
  load_w<W>(k1, false, e, k);
  load_w<W>(v, v_bf16, e, vv);
#pragma unroll
  for (int j = 0; j < W; j++) {
    const float k2 = sde_drift_one(velocity_of<M>(P, vv[j], p[j]), p[j], rar, var, diff);
    o[j] = y[j] + hdt * (k[j] + k2);
  }
  store_w<W>(out, e, o);
}

template <bool M>
__global__ __launch_bounds__(256) void sde_heun_correct_kernel(const float* __restrict__ xhat, const float* __restrict__ xp, const float* __restrict__ k1, const void* v,
                                                               int v_bf16, float* __restrict__ out, size_t n, size_t nq, float rar, float var, float diff, float hdt,
                                                               terms_arg<M> P) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { heun_correct_at<W, M>(xhat, xp, k1, v, v_bf16, out, e, rar, var, diff, hdt, P); });
}

// Tweedie: x / a + c * ((rar * v - x) / var).  Euler: x + (v * h), the product rounded to bf16 when v is bf16 (`bf16 tensor * python float` stays bf16).
// M (a noise / score model's output m): Tweedie takes Transport.get_score -- m / nsig (f32) or m itself, and then c * m is a 0-d f32 tensor times a tensor of m's
// type: a bf16 m makes it a bf16 product (c cast to bf16, the f32 product rounded to bf16) before it meets x / a --; Euler takes the converted velocity, which is f32 whatever m is.
template <int W, bool M>
__device__ __forceinline__ void last_step_at(const float* __restrict__ x, const void* v, int v_bf16, float* __restrict__ out, size_t e, int mode, float a, float c,
                                             float rar, float var, float h, const terms_arg<M>& P) {
  float y[W], vv[W], o[W];
  load_w<W>(x, false, e, y);
  load_w<W>(v, v_bf16, e, vv);
#pragma unroll
  for (int j = 0; j < W; j++) {
    if (mode == DMVAE_LAST_STEP_TWEEDIE) {
      if constexpr (M) {
        const bool both_bf16 = v_bf16 && P.kind == DMVAE_MODEL_SCORE;      // a bf16 product: the 0-d factor is cast to the result type first
        float p = (both_bf16 ? (float)(bf16)c : c) * model_score_one(P, vv[j]);
        if (both_bf16) p = (float)(bf16)p;
        o[j] = y[j] / a + p;
      } else {
        const float score = (rar * vv[j] - y[j]) / var;
        o[j] = y[j] / a + c * score;
      }
    } else {
      float p = velocity_of<M>(P, vv[j], y[j]) * h;
      if constexpr (!M) {
        if (v_bf16) p = (float)(bf16)p;
      }
      o[j] = y[j] + p;
    }
  }
  store_w<W>(out, e, o);
}

template <bool M>      // M: rar and var are not read
__global__ __launch_bounds__(256) void sde_last_step_kernel(const float* __restrict__ x, const void* v, int v_bf16, float* __restrict__ out, size_t n, size_t nq, int mode,
                                                            float a, float c, float rar, float var, float h, terms_arg<M> P) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { last_step_at<W, M>(x, v, v_bf16, out, e, mode, a, c, rar, var, h, P); });
}

// v alone, f32: the drift of the probability-flow ODE (Transport.get_drift) for a noise / score model
template <int W>
__device__ __forceinline__ void model_velocity_at(const float* __restrict__ x, const void* m, int m_bf16, const dmvae_model_terms& P, float* __restrict__ out, size_t e) {
  float y[W], mv[W], o[W];
  load_w<W>(x, false, e, y);
  load_w<W>(m, m_bf16, e, mv);
#pragma unroll
  for (int j = 0; j < W; j++) o[j] = model_velocity_one(P, mv[j], y[j]);
  store_w<W>(out, e, o);
}

__global__ __launch_bounds__(256) void model_velocity_kernel(const float* __restrict__ x, const void* m, int m_bf16, dmvae_model_terms P, float* __restrict__ out, size_t n,
                                                             size_t nq) {
  quads_then_tail(n, nq, [&](auto W, size_t e) { model_velocity_at<W>(x, m, m_bf16, P, out, e); });
}

// ---- autoguidance (LightningDiT.forward_with_autoguidance, lightningdit.py:450-465) ------------------------------------------------------------------------

// eps [n][c_eps][hw], ag [n][c_ag][hw] -> dst [2][n][k][hw]: the first k channels of every sample, g = ag + scale * (eps - ag) where lo <= t[0] <= hi (read on the
// device), eps itself elsewhere; both halves of dst receive it.  Rounding as cfg_one: a bf16 tensor rounds after each of the three ops.
template <typename T, int W>
__device__ __forceinline__ void autoguidance_at(const T* __restrict__ eps, const T* __restrict__ ag, T* __restrict__ dst, size_t e, size_t half, size_t per, size_t per_eps,
                                                size_t per_ag, float scale, bool inside) {
  const size_t s = e / per, r = e - s * per;                 // sample, offset inside its first k channels (W == 4: per % 4 == 0, a quad stays in one sample)
  float a[W], b[W];
  load_w<W>(eps, sizeof(T) == 2, s * per_eps + r, a);
  if (inside) {
    load_w<W>(ag, sizeof(T) == 2, s * per_ag + r, b);
#pragma unroll
    for (int j = 0; j < W; j++) a[j] = cfg_one<T>(a[j], b[j], scale, false);
  }
  store_w<W>(dst, e, a);
  store_w<W>(dst + half, e, a);
}

template <typename T>
__global__ __launch_bounds__(256) void autoguidance_combine_kernel(const T* __restrict__ eps, const T* __restrict__ ag, T* __restrict__ dst, size_t half, size_t nq,
                                                                   size_t per, size_t per_eps, size_t per_ag, float scale, const float* __restrict__ t, float lo,
                                                                   float hi) {
  const float t0 = t[0];
  const bool inside = t0 >= lo && t0 <= hi;
  quads_then_tail(half, nq, [&](auto W, size_t e) { autoguidance_at<T, W>(eps, ag, dst, e, half, per, per_eps, per_ag, scale, inside); });
}

// ---- host side: the quads decision, the launch, the entry points ----------------------------------------------------------------------------------------------

constexpr int kErrMaxParts = 1024;

inline int ode_grid(size_t n, size_t nq, int cap) {
  const size_t work = nq + (n - 4 * nq);                    // quads, then the scalar tail
  const size_t g = (work + 255) / 256;
  return (int)(g < (size_t)cap ? (g > 0 ? g : 1) : (size_t)cap);
}

inline bool aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

struct typed_ptr { const void* p; int is_bf16; };

// How many quads a pass over n elements may take: n / 4 when every pointer is aligned for them -- f32 arrays (f32s, and T's f32 terms) to 16 bytes, bf16 arrays to 8;
// NULL is an absent array --, else none
inline size_t ode_quads(size_t n, const dmvae_ode_terms* T, std::initializer_list<const void*> f32s, std::initializer_list<typed_ptr> typed = {}) {
  bool ok = true;
  for (const void* p : f32s) ok = ok && aligned(p, 16);
  for (const typed_ptr& t : typed) ok = ok && aligned(t.p, t.is_bf16 ? 8 : 16);
  if (T)
    for (int j = 0; j < T->nk; j++) ok = ok && aligned(T->k[j], ((T->k_bf16 >> j) & 1) ? 8 : 16);
  return ok ? n / 4 : 0;
}

// One pass: ode_grid(n, nq, cap) workgroups of 256 threads; every argument converted to the kernel's parameter type (void* -> float*, int -> bool, ...)
template <class... P, class... A>
inline int launch(void (*kernel)(P...), hipStream_t stream, size_t n, size_t nq, int cap, A... args) {
  hipLaunchKernelGGL(kernel, dim3(ode_grid(n, nq, cap)), dim3(256), 0, stream, (P)args...);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

inline bool terms_ok(const dmvae_ode_terms* T) {
  if (!T || T->nk < 1 || T->nk > DMVAE_ODE_MAX_TERMS) return false;
  for (int j = 0; j < T->nk; j++)
    if (!T->k[j]) return false;
  return true;
}

inline bool model_terms_ok(const dmvae_model_terms* P) { return P && (P->kind == DMVAE_MODEL_NOISE || P->kind == DMVAE_MODEL_SCORE); }

// The model-consuming passes, behind their velocity and `_m` entry points: terms NULL -> the velocity instantiation

static int euler_step(const void* x, const void* v, int v_bf16, const dmvae_model_terms* terms_or_null, const void* w, void* x_out, void* mean_out, size_t n, float rar,
                      float var, float diff, float dt, float sq2d, float sqdt, hipStream_t stream) {
  const size_t nq = ode_quads(n, nullptr, {x, w, x_out, mean_out}, {{v, v_bf16}});
  return terms_or_null ? launch(sde_euler_kernel<true>, stream, n, nq, 2048, x, v, v_bf16 != 0, w, x_out, mean_out, n, nq, rar, var, diff, dt, sq2d, sqdt, *terms_or_null)
                       : launch(sde_euler_kernel<false>, stream, n, nq, 2048, x, v, v_bf16 != 0, w, x_out, mean_out, n, nq, rar, var, diff, dt, sq2d, sqdt, no_terms{});
}

static int heun_predict(const void* xhat, const void* v1, int v_bf16, const dmvae_model_terms* terms_or_null, void* k1, void* xp, size_t n, float rar, float var,
                        float diff, float dt, hipStream_t stream) {
  const size_t nq = ode_quads(n, nullptr, {xhat, k1, xp}, {{v1, v_bf16}});
  return terms_or_null ? launch(sde_heun_predict_kernel<true>, stream, n, nq, 2048, xhat, v1, v_bf16 != 0, k1, xp, n, nq, rar, var, diff, dt, *terms_or_null)
                       : launch(sde_heun_predict_kernel<false>, stream, n, nq, 2048, xhat, v1, v_bf16 != 0, k1, xp, n, nq, rar, var, diff, dt, no_terms{});
}

static int heun_correct(const void* xhat, const void* xp, const void* k1, const void* v2, int v_bf16, const dmvae_model_terms* terms_or_null, void* x_out, size_t n,
                        float rar2, float var2, float diff2, float half_dt, hipStream_t stream) {
  const size_t nq = ode_quads(n, nullptr, {xhat, xp, k1, x_out}, {{v2, v_bf16}});
  return terms_or_null ? launch(sde_heun_correct_kernel<true>, stream, n, nq, 2048, xhat, xp, k1, v2, v_bf16 != 0, x_out, n, nq, rar2, var2, diff2, half_dt, *terms_or_null)
                       : launch(sde_heun_correct_kernel<false>, stream, n, nq, 2048, xhat, xp, k1, v2, v_bf16 != 0, x_out, n, nq, rar2, var2, diff2, half_dt, no_terms{});
}

static int last_step(const void* x, const void* v, int v_bf16, const dmvae_model_terms* terms_or_null, void* out, size_t n, int mode, float a, float c, float rar,
                     float var, float h, hipStream_t stream) {
  const size_t nq = ode_quads(n, nullptr, {x, out}, {{v, v_bf16}});
  return terms_or_null ? launch(sde_last_step_kernel<true>, stream, n, nq, 2048, x, v, v_bf16 != 0, out, n, nq, mode, a, c, rar, var, h, *terms_or_null)
                       : launch(sde_last_step_kernel<false>, stream, n, nq, 2048, x, v, v_bf16 != 0, out, n, nq, mode, a, c, rar, var, h, no_terms{});
}

}  // namespace dmvae_sampler

using namespace dmvae_sampler;

extern "C" int dmvae_sde_euler_step(const void* x, const void* v, int v_is_bf16, const void* w, void* x_out, void* mean_out, size_t n, float rar,
                                    float var, float diff, float dt, float sqrt_2diff, float sqrt_dt, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && v && (x_out || mean_out) && n > 0, "sde_euler_step: bad argument (x, v, x_out or mean_out non-NULL, n > 0)");
  return euler_step(x, v, v_is_bf16, nullptr, w, x_out, mean_out, n, rar, var, diff, dt, sqrt_2diff, sqrt_dt, stream);
}

extern "C" int dmvae_image_to_u8(const void* y, void* out, size_t npix, int c, int c_stride, int round_bf16, hipStream_t stream) {
  DMVAE_CHECK_ARG(y && out && npix > 0 && c > 0 && c <= c_stride, "image_to_u8: bad argument");
  const int grid = (int)((npix + 255) / 256 < 4096 ? (npix + 255) / 256 : 4096);
  hipLaunchKernelGGL(image_to_u8_kernel, dim3(grid), dim3(256), 0, stream, (const float*)y, (uint8_t*)out, npix, c, c_stride, round_bf16);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_ode_rk_combine(const void* y0, const dmvae_ode_terms* terms, void* out, size_t n, int round_bf16, hipStream_t stream) {
  DMVAE_CHECK_ARG(terms_ok(terms) && out && n > 0, "ode_rk_combine: bad argument (1 <= nk <= %d non-NULL k, out, n > 0)", DMVAE_ODE_MAX_TERMS);
  const size_t nq = ode_quads(n, terms, {y0, out});
  return launch(ode_rk_combine_kernel, stream, n, nq, 2048, y0, *terms, out, n, nq, round_bf16);
}

extern "C" size_t dmvae_ode_error_ratio_workspace(size_t n) {
  (void)n;
  return (size_t)kErrMaxParts * (sizeof(double) + sizeof(int));
}

extern "C" int dmvae_ode_error_ratio(const void* y0, const void* y1, const dmvae_ode_terms* terms, float atol, float rtol, int round_bf16, void* err_out,
                                     void* workspace, void* result, size_t n, hipStream_t stream) {
  DMVAE_CHECK_ARG(y0 && y1 && terms_ok(terms) && workspace && result && n > 0 && aligned(workspace, 8) && aligned(result, 8),
                  "ode_error_ratio: bad argument");
  const size_t nq = ode_quads(n, terms, {y0, y1, err_out});
  double* part = (double*)workspace;
  int* part_bad = (int*)(part + kErrMaxParts);
  if (const int rc = launch(ode_err_partial_kernel, stream, n, nq, kErrMaxParts, y0, y1, *terms, err_out, part, part_bad, n, nq, atol, rtol, round_bf16)) return rc;
  hipLaunchKernelGGL(ode_err_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)part, (const int*)part_bad, ode_grid(n, nq, kErrMaxParts), n, result);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_ode_dense_output(const void* y0, const void* y1, const void* y_mid, const void* f0, const void* f1, int f_bf16, float dt, float x,
                                      void* out, size_t n, hipStream_t stream) {
  DMVAE_CHECK_ARG(y0 && y1 && y_mid && f0 && f1 && out && n > 0, "ode_dense_output: bad argument");
  const size_t nq = ode_quads(n, nullptr, {y0, y1, y_mid, out}, {{f0, f_bf16 & 1}, {f1, f_bf16 & 2}});
  return launch(ode_dense_kernel, stream, n, nq, 2048, y0, y1, y_mid, f0, f1, f_bf16, dt, x, out, n, nq);
}

extern "C" int dmvae_ode_hutchinson_pack(const void* v, int v_is_bf16, const void* g, const void* eps, void* k_x, void* k_logp, int batch, size_t per_sample,
                                         hipStream_t stream) {
  DMVAE_CHECK_ARG(v && g && eps && k_x && k_logp && batch > 0 && batch <= 65535 && per_sample > 0, "ode_hutchinson_pack: bad argument");
  const bool quads = per_sample % 4 == 0 && ode_quads(per_sample, nullptr, {g, eps, k_x}, {{v, v_is_bf16}}) > 0;      // every sample starts on a quad and holds whole ones
  hipLaunchKernelGGL(ode_hutchinson_pack_kernel, dim3(batch), dim3(1024), 0, stream, v, v_is_bf16, (const float*)g, (const float*)eps, (float*)k_x, (float*)k_logp,
                     per_sample, (int)quads);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_cfg_combine(const void* out2n, int is_bf16, void* dst, int n, int channels, size_t hw, int k, float scale, const void* t_or_null,
                                 float interval_start, hipStream_t stream) {
  DMVAE_CHECK_ARG(out2n && dst, "cfg_combine: out2n and dst must not be NULL");
  DMVAE_CHECK_ARG(dst != out2n, "cfg_combine: dst must not alias out2n");
  DMVAE_CHECK_ARG(n > 0 && channels > 0 && hw > 0 && k >= 0, "cfg_combine: bad argument (n > 0, channels > 0, hw > 0, k >= 0; got n %d, channels %d, hw %zu, k %d)", n,
                  channels, hw, k);
  if (k > channels) k = channels;
  const size_t half = (size_t)n * (size_t)channels * hw;
  const size_t nq = hw % 4 == 0 ? ode_quads(half, nullptr, {}, {{out2n, is_bf16}, {dst, is_bf16}}) : 0;      // hw % 4 == 0 keeps a quad inside one channel and the second half as aligned as the first
  return is_bf16 ? launch(cfg_combine_kernel<bf16>, stream, half, nq, 2048, out2n, dst, half, nq, hw, channels, k, scale, t_or_null, interval_start)
                 : launch(cfg_combine_kernel<float>, stream, half, nq, 2048, out2n, dst, half, nq, hw, channels, k, scale, t_or_null, interval_start);
}

extern "C" int dmvae_sde_heun_perturb(const void* x, const void* w, void* xhat, size_t n, float sqrt_2diff, float sqrt_dt, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && w && xhat && n > 0, "sde_heun_perturb: bad argument (x, w, xhat non-NULL, n > 0)");
  const size_t nq = ode_quads(n, nullptr, {x, w, xhat});
  return launch(sde_heun_perturb_kernel, stream, n, nq, 2048, x, w, xhat, n, nq, sqrt_2diff, sqrt_dt);
}

extern "C" int dmvae_sde_heun_predict(const void* xhat, const void* v1, int v_is_bf16, void* k1, void* xp, size_t n, float rar, float var, float diff, float dt,
                                      hipStream_t stream) {
  DMVAE_CHECK_ARG(xhat && v1 && k1 && xp && n > 0, "sde_heun_predict: bad argument (xhat, v1, k1, xp non-NULL, n > 0)");
  return heun_predict(xhat, v1, v_is_bf16, nullptr, k1, xp, n, rar, var, diff, dt, stream);
}

extern "C" int dmvae_sde_heun_correct(const void* xhat, const void* xp, const void* k1, const void* v2, int v_is_bf16, void* x_out, size_t n, float rar2, float var2,
                                      float diff2, float half_dt, hipStream_t stream) {
  DMVAE_CHECK_ARG(xhat && xp && k1 && v2 && x_out && n > 0, "sde_heun_correct: bad argument (xhat, xp, k1, v2, x_out non-NULL, n > 0)");
  return heun_correct(xhat, xp, k1, v2, v_is_bf16, nullptr, x_out, n, rar2, var2, diff2, half_dt, stream);
}

extern "C" int dmvae_sde_last_step(const void* x, const void* v, int v_is_bf16, void* out, size_t n, int mode, float a, float c, float rar, float var, float h,
                                   hipStream_t stream) {
  DMVAE_CHECK_ARG(x && v && out && n > 0, "sde_last_step: bad argument (x, v, out non-NULL, n > 0)");
  DMVAE_CHECK_ARG(mode == DMVAE_LAST_STEP_TWEEDIE || mode == DMVAE_LAST_STEP_EULER, "sde_last_step: mode must be DMVAE_LAST_STEP_TWEEDIE or _EULER, got %d", mode);
  return last_step(x, v, v_is_bf16, nullptr, out, n, mode, a, c, rar, var, h, stream);
}

extern "C" int dmvae_autoguidance_combine(const void* eps, int c_eps, const void* ag, int c_ag, int is_bf16, void* dst, int n, size_t hw, int k, float scale,
                                          const void* t, float lo, float hi, hipStream_t stream) {
  DMVAE_CHECK_ARG(eps && ag && dst && t, "autoguidance_combine: eps, ag, dst and t must not be NULL");
  DMVAE_CHECK_ARG(dst != eps && dst != ag, "autoguidance_combine: dst must not alias eps or ag");
  DMVAE_CHECK_ARG(n > 0 && hw > 0 && k > 0 && k <= c_eps && k <= c_ag,
                  "autoguidance_combine: bad argument (n > 0, hw > 0, 0 < k <= channels of eps and ag; got n %d, hw %zu, k %d, channels %d and %d)", n, hw, k, c_eps, c_ag);
  const size_t per = (size_t)k * hw, per_eps = (size_t)c_eps * hw, per_ag = (size_t)c_ag * hw, half = (size_t)n * per;
  const bool whole = per % 4 == 0 && per_eps % 4 == 0 && per_ag % 4 == 0;      // every sample's first k channels start on a quad and hold whole quads, in all three arrays
  const size_t nq = whole ? ode_quads(half, nullptr, {}, {{eps, is_bf16}, {ag, is_bf16}, {dst, is_bf16}}) : 0;
  return is_bf16 ? launch(autoguidance_combine_kernel<bf16>, stream, half, nq, 2048, eps, ag, dst, half, nq, per, per_eps, per_ag, scale, t, lo, hi)
                 : launch(autoguidance_combine_kernel<float>, stream, half, nq, 2048, eps, ag, dst, half, nq, per, per_eps, per_ag, scale, t, lo, hi);
}

extern "C" int dmvae_sde_euler_step_m(const void* x, const void* m, int m_is_bf16, const dmvae_model_terms* terms, const void* w, void* x_out, void* mean_out, size_t n,
                                      float rar, float var, float diff, float dt, float sqrt_2diff, float sqrt_dt, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && m && (x_out || mean_out) && n > 0, "sde_euler_step_m: bad argument (x, m, x_out or mean_out non-NULL, n > 0)");
  DMVAE_CHECK_ARG(model_terms_ok(terms), "sde_euler_step_m: terms->kind must be DMVAE_MODEL_NOISE or DMVAE_MODEL_SCORE");
  return euler_step(x, m, m_is_bf16, terms, w, x_out, mean_out, n, rar, var, diff, dt, sqrt_2diff, sqrt_dt, stream);
}

extern "C" int dmvae_sde_heun_predict_m(const void* xhat, const void* m1, int m_is_bf16, const dmvae_model_terms* terms, void* k1, void* xp, size_t n, float rar, float var,
                                        float diff, float dt, hipStream_t stream) {
  DMVAE_CHECK_ARG(xhat && m1 && k1 && xp && n > 0, "sde_heun_predict_m: bad argument (xhat, m1, k1, xp non-NULL, n > 0)");
  DMVAE_CHECK_ARG(model_terms_ok(terms), "sde_heun_predict_m: terms->kind must be DMVAE_MODEL_NOISE or DMVAE_MODEL_SCORE");
  return heun_predict(xhat, m1, m_is_bf16, terms, k1, xp, n, rar, var, diff, dt, stream);
}

extern "C" int dmvae_sde_heun_correct_m(const void* xhat, const void* xp, const void* k1, const void* m2, int m_is_bf16, const dmvae_model_terms* terms2, void* x_out,
                                        size_t n, float rar2, float var2, float diff2, float half_dt, hipStream_t stream) {
  DMVAE_CHECK_ARG(xhat && xp && k1 && m2 && x_out && n > 0, "sde_heun_correct_m: bad argument (xhat, xp, k1, m2, x_out non-NULL, n > 0)");
  DMVAE_CHECK_ARG(model_terms_ok(terms2), "sde_heun_correct_m: terms2->kind must be DMVAE_MODEL_NOISE or DMVAE_MODEL_SCORE");
  return heun_correct(xhat, xp, k1, m2, m_is_bf16, terms2, x_out, n, rar2, var2, diff2, half_dt, stream);
}

extern "C" int dmvae_sde_last_step_m(const void* x, const void* m, int m_is_bf16, const dmvae_model_terms* terms, void* out, size_t n, int mode, float a, float c, float h,
                                     hipStream_t stream) {
  DMVAE_CHECK_ARG(x && m && out && n > 0, "sde_last_step_m: bad argument (x, m, out non-NULL, n > 0)");
  DMVAE_CHECK_ARG(model_terms_ok(terms), "sde_last_step_m: terms->kind must be DMVAE_MODEL_NOISE or DMVAE_MODEL_SCORE");
  DMVAE_CHECK_ARG(mode == DMVAE_LAST_STEP_TWEEDIE || mode == DMVAE_LAST_STEP_EULER, "sde_last_step_m: mode must be DMVAE_LAST_STEP_TWEEDIE or _EULER, got %d", mode);
  return last_step(x, m, m_is_bf16, terms, out, n, mode, a, c, 0.f, 1.f, h, stream);
}

extern "C" int dmvae_model_velocity(const void* x, const void* m, int m_is_bf16, const dmvae_model_terms* terms, void* out, size_t n, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && m && out && n > 0, "model_velocity: bad argument (x, m, out non-NULL, n > 0)");
  DMVAE_CHECK_ARG(model_terms_ok(terms), "model_velocity: terms->kind must be DMVAE_MODEL_NOISE or DMVAE_MODEL_SCORE");
  const size_t nq = ode_quads(n, nullptr, {x, out}, {{m, m_is_bf16}});
  return launch(model_velocity_kernel, stream, n, nq, 2048, x, m, m_is_bf16 != 0, *terms, out, n, nq);
}
