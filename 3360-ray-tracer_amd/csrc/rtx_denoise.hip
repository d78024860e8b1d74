// rtx_denoise.hip — the edge-avoiding a-trous wavelet filter; see rtx_denoise.h and DESIGN.md §4b.
//
// Working set per pixel: colour + variance {r, g, b, var} (ping-pong), one guide record {nx, ny,
// nz, depth} and the albedo, a float4 each, so every tap is two 16-byte loads.  Iteration k reads
// the 5 x 5 taps at step 2^k.  At steps 1 and 2 the taps of a 32 x 8 block overlap almost
// entirely, so the block stages its tile and halo in LDS once; from step 4 on neighbouring lanes'
// taps are neighbouring pixels of other rows and columns, which the L2 serves as plain coalesced
// loads.  One lane per pixel, no atomics: a pixel's sums run in tap order, whatever the launch.
#include "rtx_denoise.h"

namespace rtxdn {
namespace {

constexpr int kBlock = 256;
constexpr int kTX = 32, kTY = 8;  // a block's pixels (kTX * kTY == kBlock)
constexpr float kLog2e = 1.44269504088896340736f;

__device__ __forceinline__ float lum(float r, float g, float b) {
  return fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r));
}
__device__ __forceinline__ float4 albedo_floor(float4 a) {
  return make_float4(fmaxf(a.x, kAlbedoFloor), fmaxf(a.y, kAlbedoFloor), fmaxf(a.z, kAlbedoFloor), 0.0f);
}

__global__ __launch_bounds__(kBlock) void k_dn_guides(const double* __restrict__ normal,
                                                      const double* __restrict__ depth,
                                                      const double* __restrict__ albedo, int64_t n,
                                                      float4* __restrict__ guide, float4* __restrict__ alb) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  guide[i] = make_float4((float)normal[3 * i], (float)normal[3 * i + 1], (float)normal[3 * i + 2], (float)depth[i]);
  alb[i] = make_float4((float)albedo[3 * i], (float)albedo[3 * i + 1], (float)albedo[3 * i + 2], 0.0f);
}

__global__ __launch_bounds__(kBlock) void k_dn_prologue(const double* __restrict__ rgb, const double* __restrict__ var,
                                                        const float4* __restrict__ alb, int64_t n, int demodulate,
                                                        float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float4 c = make_float4((float)rgb[3 * i], (float)rgb[3 * i + 1], (float)rgb[3 * i + 2], var ? (float)var[i] : 0.0f);
  if (demodulate) {
    const float4 a = albedo_floor(alb[i]);
    c.x = c.x / a.x, c.y = c.y / a.y, c.z = c.z / a.z;
  }
  out[i] = c;
}

__global__ __launch_bounds__(kBlock) void k_dn_epilogue(const float4* __restrict__ in, const float4* __restrict__ alb,
                                                        int64_t n, int demodulate, double* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float4 c = in[i];
  if (demodulate) {
    const float4 a = albedo_floor(alb[i]);
    c.x = c.x * a.x, c.y = c.y * a.y, c.z = c.z * a.z;
  }
  rgb[3 * i] = (double)c.x, rgb[3 * i + 1] = (double)c.y, rgb[3 * i + 2] = (double)c.z;
}

// What a pixel's taps are weighed against: its own guide, luminance and the two exponents' scales
// (log2 e folded in: the weights go through exp2).
struct Centre {
  float nx, ny, nz, z, l;
  bool hit;
  float kz, kl, power;  // log2(e) / sigma_depth; log2(e) / (sigma_color g_p + 1e-6); normal_power
};
struct Sums {
  float r, g, b, v, w;
};

// One tap q != p: w = h w_n w_z w_l, 0 outside the grid or across the hit / miss boundary.
// w_n = pow(max(0, n_p . n_q), power) as exp2(power log2(.)): 0 at a dot of 0 exactly.
__device__ __forceinline__ void tap(const Centre& P, float4 c, float4 g, float hh, bool inside, Sums& s) {
  const bool hq = g.w > 0.0f, both = P.hit && hq;
  const float dot = fmaxf(0.0f, fmaf(P.nz, g.z, fmaf(P.ny, g.y, P.nx * g.x)));
  const float wn = both ? __builtin_amdgcn_exp2f(P.power * __builtin_amdgcn_logf(dot)) : 1.0f;
  const float ez = both ? fabsf(P.z - g.w) * P.kz * __builtin_amdgcn_rcpf(fmaxf(P.z, g.w)) : 0.0f;
  const float el = fabsf(P.l - lum(c.x, c.y, c.z)) * P.kl;
  float w = hh * wn * __builtin_amdgcn_exp2f(-(ez + el));
  w = (inside && hq == P.hit) ? w : 0.0f;
  s.r = fmaf(w, c.x, s.r), s.g = fmaf(w, c.y, s.g), s.b = fmaf(w, c.z, s.b);
  s.v = fmaf(w * w, c.w, s.v);
  s.w += w;
}

__device__ __forceinline__ constexpr float h5(int d) { return (d == 0 ? 6.0f : (d == 1 || d == -1) ? 4.0f : 1.0f) / 16.0f; }
__device__ __forceinline__ constexpr float h3(int d) { return d == 0 ? 2.0f : 1.0f; }

// S > 0: step S with the block's tile in LDS; S == 0: step `step` from global memory.
template <int S>
__global__ __launch_bounds__(kBlock) void k_atrous(const float4* __restrict__ cin, const float4* __restrict__ guide,
                                                      float4* __restrict__ cout, int W, int H, int nbx, int step,
                                                      int has_var, float power, float kz, float sigma_color) {
  constexpr int HALO = 2 * S, TW = kTX + 2 * HALO, TH = kTY + 2 * HALO;
  __shared__ float4 tc[S ? TW * TH : 1], tg[S ? TW * TH : 1];
  const int tx = threadIdx.x % kTX, ty = threadIdx.x / kTX;
  const int bx = (int)(blockIdx.x % (unsigned)nbx) * kTX, by = (int)(blockIdx.x / (unsigned)nbx) * kTY;  // nbx blocks per row
  const int x = bx + tx, y = by + ty;
  if (S) {
    for (int i = threadIdx.x; i < TW * TH; i += kBlock) {
      const int gx = bx - HALO + i % TW, gy = by - HALO + i / TW;
      const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
      const size_t q = (size_t)(in ? gy : 0) * W + (in ? gx : 0);
      const float4 c = cin[q], g = guide[q];
      tc[i] = in ? c : make_float4(0, 0, 0, 0);
      tg[i] = in ? g : make_float4(0, 0, 0, 0);
    }
    __syncthreads();
  }
  if (x >= W || y >= H) return;
  const int lp = (ty + HALO) * TW + tx + HALO;  // this pixel in the tile
  const size_t p = (size_t)y * W + x;
  const float4 cp = S ? tc[lp] : cin[p], gp = S ? tg[lp] : guide[p];
  float gsd = 1.0f;  // g_p: the standard deviation the colour distance is measured in
  if (has_var) {     // the 3 x 3 Gaussian of var around p (step 1), taps outside skipped
    float sv = 0.0f, sk = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = x + dx, qy = y + dy;
        const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
        const float v = S ? tc[lp + dy * TW + dx].w : cin[(size_t)(in ? qy : y) * W + (in ? qx : x)].w;
        const float k = in ? h3(dx) * h3(dy) : 0.0f;
        sv = fmaf(k, v, sv), sk += k;
      }
    gsd = sqrtf(fmaxf(0.0f, sv / sk));
  }
  Centre P;
  P.nx = gp.x, P.ny = gp.y, P.nz = gp.z, P.z = gp.w, P.hit = gp.w > 0.0f;
  P.l = lum(cp.x, cp.y, cp.z);
  P.kz = kz, P.kl = kLog2e / fmaf(sigma_color, gsd, 1e-6f), P.power = power;
  const float w0 = h5(0) * h5(0);  // the centre tap's weight, whatever its guide
  Sums s{w0 * cp.x, w0 * cp.y, w0 * cp.z, w0 * w0 * cp.w, w0};
  const int st = S ? S : step;
  // a row of taps at a time: five rows of loads in flight at once would not fit the registers
#pragma unroll 1
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      if (dx == 0 && dy == 0) continue;
      const int qx = x + dx * st, qy = y + dy * st;
      const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
      float4 c, g;
      if (S) {
        const int lq = lp + dy * S * TW + dx * S;
        c = tc[lq], g = tg[lq];
      } else {  // an address inside the grid either way: the loads need no branch
        const size_t q = (size_t)(in ? qy : y) * W + (in ? qx : x);
        c = cin[q], g = guide[q];
      }
      tap(P, c, g, h5(dx) * h5(dy), in, s);
    }
  cout[p] = make_float4(s.r / s.w, s.g / s.w, s.b / s.w, s.v / (s.w * s.w));
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t pack_guides(const double* d_normal, const double* d_depth, const double* d_albedo, int64_t npix,
                       float4* guide, float4* albedo, hipStream_t s) {
  if (npix <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dn_guides, dim3(blocks_of(npix)), dim3(kBlock), 0, s, d_normal, d_depth, d_albedo, npix, guide,
                     albedo);
  return hipGetLastError();
}

hipError_t filter(int32_t w, int32_t h, const double* d_rgb, const double* d_var, const float4* guide,
                  const float4* albedo, float4* work0, float4* work1, const FilterParams& p, double* d_out,
                  hipStream_t s) {
  const int64_t npix = (int64_t)w * h;
  if (npix <= 0) return hipSuccess;
  if (p.iterations == 0)
    return d_out == d_rgb ? hipSuccess
                          : hipMemcpyAsync(d_out, d_rgb, (size_t)npix * 3 * sizeof(double), hipMemcpyDeviceToDevice, s);
  const int demod = (p.flags & kDemodulate) ? 1 : 0, has_var = d_var ? 1 : 0;
  hipLaunchKernelGGL(k_dn_prologue, dim3(blocks_of(npix)), dim3(kBlock), 0, s, d_rgb, d_var, albedo, npix, demod,
                     work0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int nbx = (w + kTX - 1) / kTX;  // a 1-D grid: an image one pixel wide has up to 2^28 block rows
  const dim3 grid((unsigned)((int64_t)nbx * ((h + kTY - 1) / kTY)));
  const float kz = kLog2e / p.sigma_depth;
  float4* buf[2] = {work0, work1};
  for (int k = 0; k < p.iterations; k++) {
    const float4* src = buf[k & 1];
    float4* dst = buf[(k + 1) & 1];
    const int step = 1 << k;
    if (step == 1)
      hipLaunchKernelGGL(k_atrous<1>, grid, dim3(kBlock), 0, s, src, guide, dst, w, h, nbx, step, has_var,
                         p.normal_power, kz, p.sigma_color);
    else if (step == 2)
      hipLaunchKernelGGL(k_atrous<2>, grid, dim3(kBlock), 0, s, src, guide, dst, w, h, nbx, step, has_var,
                         p.normal_power, kz, p.sigma_color);
    else
      hipLaunchKernelGGL(k_atrous<0>, grid, dim3(kBlock), 0, s, src, guide, dst, w, h, nbx, step, has_var,
                         p.normal_power, kz, p.sigma_color);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_dn_epilogue, dim3(blocks_of(npix)), dim3(kBlock), 0, s, (const float4*)buf[p.iterations & 1],
                     albedo, npix, demod, d_out);
  return hipGetLastError();
}

}  // namespace rtxdn
