// rtx_film.h — a film: the per-pixel render state (PixelSoA) kept between calls, so a frame is
// rendered in steps, shown in between, saved and continued (rtx_film_*, include/rtx.h).
// Here: the blob a film is saved as (header + state arrays, DESIGN.md "Film"), its host-side
// check, and the film's own kernels: resolve on demand, state -> blob body and back.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "rtx_denoise.h"
#include "rtx_kernels.h"

namespace rtxd {

// ---- the saved blob -----------------------------------------------------------------------
// Little-endian.  Header (kFilmHeaderBytes), then the state arrays in this order, each
// channel-major as on the device (value of channel c of pixel p at c * npix + p):
//   sum      3 x npix f64
//   mean     3 x npix f64   adaptive films only
//   m2       3 x npix f64   adaptive films only
//   samples      npix i32
//   conv         npix u8    adaptive films only
constexpr uint32_t kFilmVersion = 1;
constexpr char kFilmMagic[8] = {'R', 'T', 'X', 'F', 'I', 'L', 'M', '\0'};
struct FilmHeader {
  char magic[8];          //   0  "RTXFILM\0"
  uint32_t version;       //   8  kFilmVersion
  uint32_t header_bytes;  //  12  kFilmHeaderBytes
  int32_t W, H;           //  16  the image
  int32_t stripes;        //  24  the pixel map: 0 rectangle, 1 interleaved row stripes
  int32_t x0, y0, w, h;   //  28  rectangle (stripes: 0, 0, W, the stripes' rows)
  int32_t srows, sidx, scount;  // 44  stripes: rows per stripe, index, count (rectangle: 0, 0, 0)
  uint64_t seed;          //  56
  int32_t max_depth;      //  64
  int32_t adaptive;       //  68  0 / 1
  int32_t min_spp;        //  72
  int32_t sampler;        //  76  0 wavefront family (wavefront, persistent), 1 megakernel,
                          //      2 / 3 a sampled film: next-event estimation / MIS (rtx_film_create_sampled)
  double rel_threshold;   //  80
  int32_t done;           //  88  samples done (the film's budget so far)
  int32_t reserved;       //  92  0
  int64_t npix;           //  96  pixels of the map
};
constexpr uint32_t kFilmHeaderBytes = 104;
static_assert(sizeof(FilmHeader) == kFilmHeaderBytes, "FilmHeader is the blob's header, field for field");

inline size_t film_body_bytes(int64_t npix, int adaptive) {
  return (size_t)npix * (adaptive ? 9 * sizeof(double) + sizeof(int32_t) + 1 : 3 * sizeof(double) + sizeof(int32_t));
}

// Pixels of a header's map, as subset_pixels counts them; -1 with `err` naming the field.
inline int64_t film_map_pixels(const FilmHeader& h, std::string& err) {
  if (h.W <= 0 || h.H <= 0 || (int64_t)h.W * h.H > 0x7FFFFFFFll) return err = "image size", -1;
  if (h.stripes != 0 && h.stripes != 1) return err = "pixel map kind", -1;
  if (h.stripes) {
    if (h.srows <= 0 || h.scount <= 0 || h.sidx < 0 || h.sidx >= h.scount) return err = "stripe fields", -1;
    const int64_t period = (int64_t)h.srows * h.scount, first = (int64_t)h.sidx * h.srows;
    int64_t rows = 0;  // rows y with (y / srows) % scount == sidx
    for (int64_t y0 = first; y0 < h.H; y0 += period) rows += std::min<int64_t>(h.srows, h.H - y0);
    if (h.x0 != 0 || h.y0 != 0 || h.w != h.W || h.h != rows) return err = "rectangle fields of a stripe map", -1;
    return rows * h.W;
  }
  if (h.srows != 0 || h.sidx != 0 || h.scount != 0) return err = "stripe fields of a rectangle map", -1;
  if (h.x0 < 0 || h.y0 < 0 || h.w < 0 || h.h < 0 || (int64_t)h.x0 + h.w > h.W || (int64_t)h.y0 + h.h > h.H)
    return err = "rectangle", -1;
  return (int64_t)h.w * h.h;
}

// Header and length of a blob (host only).  Empty string: a well-formed film blob.
inline std::string film_blob_error(const void* blob, size_t len, FilmHeader* out = nullptr) {
  if (!blob) return "blob is NULL";
  if (len < kFilmHeaderBytes) return "truncated: shorter than the header";
  FilmHeader h;
  std::memcpy(&h, blob, sizeof h);
  if (std::memcmp(h.magic, kFilmMagic, sizeof h.magic) != 0) return "bad magic";
  if (h.version != kFilmVersion) return "unsupported format version " + std::to_string(h.version);
  if (h.header_bytes != kFilmHeaderBytes) return "bad header size";
  std::string field;
  const int64_t npix = film_map_pixels(h, field);
  if (npix < 0) return "bad " + field;
  if (npix != h.npix) return "pixel count does not match the pixel map";
  if (h.adaptive != 0 && h.adaptive != 1) return "bad adaptive flag";
  if (h.sampler < 0 || h.sampler > 3) return "bad sampler";
  if (h.sampler == 1 && h.adaptive) return "megakernel films are not adaptive";
  if (h.max_depth < 0) return "negative max_depth";
  if (h.done < 0) return "negative samples done";
  if (h.reserved != 0) return "reserved field set";
  const size_t want = kFilmHeaderBytes + film_body_bytes(npix, h.adaptive);
  if (len < want) return "truncated: " + std::to_string(len) + " bytes, " + std::to_string(want) + " expected";
  if (len > want) return "length " + std::to_string(len) + " above the " + std::to_string(want) + " bytes of its state";
  if (out) *out = h;
  return "";
}

#ifdef __HIPCC__
// The film's output at its current budget: k_resolve's arithmetic (wavefront.cc:229-235, sum /
// (float)samples per pixel; the megakernel's DefaultSampler, sum / spp with spp = samples done).
__global__ __launch_bounds__(kBlock) void k_film_resolve(PixelSoA px, int64_t npix, int sampler, int done,
                                                         double* __restrict__ rgb, int32_t* __restrict__ spp_out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  const int n = sampler == 1 ? done : px.samples[p];
  double s = 0.0;
  if (n > 0) s = sampler == 1 ? 1.0 / (double)n : 1.0 / (double)(float)n;
  for (int c = 0; c < 3; c++) rgb[3 * p + c] = n > 0 ? s * px.sum[c * npix + p] : 0.0;
  if (spp_out) spp_out[p] = n;
}

// The blob's body as typed arrays over one buffer (8-byte aligned: the doubles come first).
struct FilmBody {
  double *sum, *mean, *m2;
  int32_t* samples;
  uint8_t* conv;
};
inline FilmBody film_body_at(void* base, int64_t npix, int adaptive) {
  FilmBody b{};
  double* d = (double*)base;
  b.sum = d, d += 3 * npix;
  if (adaptive) b.mean = d, d += 3 * npix, b.m2 = d, d += 3 * npix;
  b.samples = (int32_t*)d;
  if (adaptive) b.conv = (uint8_t*)(b.samples + npix);
  return b;
}
// State -> body (to_body 1) or body -> state (0); one thread per double of a 3 x npix array.
__global__ __launch_bounds__(kBlock) void k_film_pack(PixelSoA px, FilmBody b, int64_t npix, int adaptive,
                                                      int to_body) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= 3 * npix) return;
  if (to_body) {
    b.sum[i] = px.sum[i];
    if (adaptive) b.mean[i] = px.mean[i], b.m2[i] = px.m2[i];
    if (i < npix) {
      b.samples[i] = px.samples[i];
      if (adaptive) b.conv[i] = px.conv[i];
    }
  } else {
    px.sum[i] = b.sum[i];
    if (adaptive) px.mean[i] = b.mean[i], px.m2[i] = b.m2[i];
    if (i < npix) {
      px.samples[i] = b.samples[i];
      px.conv[i] = adaptive ? (uint8_t)(b.conv[i] != 0) : (uint8_t)0;
    }
  }
}
// The variance of an adaptive film's per-pixel estimate from its running M2, as one luminance
// figure: var_c = m2_c / (n - 1) / n (0 below two samples), var = sum_c lumweight_c^2 var_c; with
// `demodulate`, divided by lum(max(albedo, floor))^2 of the film's f32 albedo record (the colour
// the filter sees is divided by that albedo).
__global__ __launch_bounds__(kBlock) void k_film_variance(PixelSoA px, int64_t npix, const float4* __restrict__ albedo,
                                                          int demodulate, double* __restrict__ var) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  const int n = px.samples[p];
  double v = 0.0;
  if (n >= 2) {
    const double vr = (px.m2[p] / (double)(n - 1)) / (double)n;
    const double vg = (px.m2[npix + p] / (double)(n - 1)) / (double)n;
    const double vb = (px.m2[2 * npix + p] / (double)(n - 1)) / (double)n;
    v = ((0.2126 * 0.2126) * vr + (0.7152 * 0.7152) * vg) + (0.0722 * 0.0722) * vb;
    if (demodulate) {
      const float4 a = albedo[p];
      const double l = (0.2126 * (double)fmaxf(a.x, rtxdn::kAlbedoFloor) + 0.7152 * (double)fmaxf(a.y, rtxdn::kAlbedoFloor)) +
                       0.0722 * (double)fmaxf(a.z, rtxdn::kAlbedoFloor);
      v = v / (l * l);
    }
  }
  var[p] = v;
}
#endif  // __HIPCC__

}  // namespace rtxd
