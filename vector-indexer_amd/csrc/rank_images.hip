// rank_images.hip — index-load time: everything the MFMA engine (rank_block.hip, rank_stream.hip) ranks an index
// from, derived once from its f32 blocks by prepare_rank_images: squared norms and their maxima, the bf16 hi/lo images
// (about the mean of the stored vectors where that pays), the hi planes' residual, the row-major coarse table, the
// sampled list spread, and the u8 / int8 / hi-natural copies of bf16-exact lists.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device_index.hpp"
#include "mfma_bf16.hpp"
#include "rank_stream.hpp"
#include "search_internal.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;

// mu (or null): the centre the ranking images are taken about (mean_kernel) — the norm of fl(v - mu) then
__global__ void slot_norms_kernel(const float4 *blocks, uint32_t dq, uint64_t nslots, float *xnorm, uint32_t *xmax_bits,
                                  const float4 *mu = nullptr) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  double acc = 0.0;  // (pad slots hold zeros: they are marked by pad_norms_kernel from the list layout afterwards)
  const float4 *p = blocks + (s / kWave) * dq * kWave + (s % kWave);
  for (uint32_t qd = 0; qd < dq; ++qd) {
    float4 v = p[(size_t)qd * kWave];
    if (mu) { const float4 m = mu[qd]; v.x -= m.x; v.y -= m.y; v.z -= m.z; v.w -= m.w; }
    acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  float out = (float)acc;
  if (out < kBig) atomicMax(xmax_bits, __float_as_uint(out));
  xnorm[s] = fminf(out, kBig);
}

// pad slots (positions len .. 64*ceil(len/64) of every list) never rank: the mask comes from the layout, not from the
// stored ids — the reference accepts ANY u64 as external_id (api.rs:57-62), 2^64-1 included
__global__ void pad_norms_kernel(const uint32_t *first_block, const uint32_t *list_len, uint32_t nlists, float *xnorm) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t l = t >> 6, j = t & 63u;
  if (l >= nlists) return;
  const uint32_t len = list_len[l], p = len + j;
  if (p < ((len + 63u) & ~63u)) xnorm[(size_t)first_block[l] * kWave + p] = kBig;  // (finite: the kernel reuses the low mantissa bits)
}

// component sums of all stored vectors (pad slots hold zeros): WG (quad, g) walks blocks g, g + G, ..., a lane per vector;
// one atomic per component and work-group.  sums: dq * 4 doubles.
__global__ void mean_kernel(const float4 *blocks, uint32_t dq, uint64_t nblocks, double *sums) {
  const uint32_t qd = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (uint64_t b = (uint64_t)blockIdx.y * 4 + wave; b < nblocks; b += (uint64_t)gridDim.y * 4) {
    const float4 v = blocks[(b * dq + qd) * 64 + lane];
    a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
  }
  for (int o = 32; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); a3 += __shfl_xor(a3, o);
  }
  if (lane == 0) {
    atomicAdd(sums + 4 * qd + 0, a0); atomicAdd(sums + 4 * qd + 1, a1);
    atomicAdd(sums + 4 * qd + 2, a2); atomicAdd(sums + 4 * qd + 3, a3);
  }
}
__global__ void sum_f32_kernel(const float *x, uint64_t n, double *out) {  // finite entries only (pad slots hold kBig)
  double a = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    if (v < 1.0e37f) a += v;
  }
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if ((threadIdx.x & 63u) == 0u) atomicAdd(out, a);
}
__global__ void max_finite_kernel(const float *x, uint64_t n, uint32_t *bits) {  // non-negative entries; pad slots (kBig) skipped
  float m = 0.0f;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    if (v < 1.0e37f) m = fmaxf(m, v);
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63u) == 0u) atomicMax(bits, __float_as_uint(m));
}
// max over the stored vectors of |x - hi(x)|^2, x = v - mu and hi = its bf16 image: what ranking from the hi planes alone
// leaves out of q.v is at most |q| times the root of this (pad slots — norm kBig in `norms` — do not count)
__global__ void trunc_residual_kernel(const float4 *blocks, uint32_t dq, uint64_t nslots, const float *norms, const float4 *mu,
                                      uint32_t *max_bits) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float out = 0.0f;
  if (s < nslots && norms[s] < 1.0e37f) {
    double acc = 0.0;
    const float4 *p = blocks + (s / kWave) * dq * kWave + (s % kWave);
    for (uint32_t qd = 0; qd < dq; ++qd) {
      float4 v = p[(size_t)qd * kWave];
      if (mu) { const float4 m = mu[qd]; v.x -= m.x; v.y -= m.y; v.z -= m.z; v.w -= m.w; }
      const float r0 = v.x - __uint_as_float(bf16_rn(v.x) << 16), r1 = v.y - __uint_as_float(bf16_rn(v.y) << 16);
      const float r2 = v.z - __uint_as_float(bf16_rn(v.z) << 16), r3 = v.w - __uint_as_float(bf16_rn(v.w) << 16);
      acc += (double)r0 * r0 + (double)r1 * r1 + (double)r2 * r2 + (double)r3 * r3;
    }
    out = (float)(acc * 1.000001);
  }
  for (int o = 32; o > 0; o >>= 1) out = fmaxf(out, __shfl_xor(out, o));
  if ((threadIdx.x & 63u) == 0u && out > 0.0f) atomicMax(max_bits, __float_as_uint(out));
}
__global__ void mean_finish_kernel(const double *sums, uint32_t dim, uint32_t dim_pad, double n, float *mu) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < dim_pad) mu[e] = e < dim ? (float)(sums[e] / n) : 0.0f;
}

// sampled spread of the lists: sums of ||v - c(list)||^2 and ||v||^2 over the first blocks of every list (one wave per list)
__global__ void list_spread_kernel(const float4 *blocks, uint32_t dq, const float4 *cent_rows, uint32_t dim, const uint32_t *first_block,
                                   const uint32_t *list_len, uint32_t nlists, uint32_t max_blocks, double *out) {
  const uint32_t l = blockIdx.x, lane = threadIdx.x;
  if (l >= nlists) return;
  const uint32_t len = list_len[l], nb = min((len + 63u) / 64u, max_blocks);
  double s_spread = 0.0, s_norm = 0.0, cnt = 0.0;
  for (uint32_t b = 0; b < nb; ++b) {
    if (b * 64u + lane >= len) continue;
    const float4 *p = blocks + ((size_t)(first_block[l] + b) * dq) * 64 + lane;
    float sp = 0.0f, nn = 0.0f;
    for (uint32_t qd = 0; qd < dim / 4; ++qd) {
      const float4 v = p[(size_t)qd * 64], c = cent_rows[(size_t)l * (dim / 4) + qd];
      sp += (v.x - c.x) * (v.x - c.x) + (v.y - c.y) * (v.y - c.y) + (v.z - c.z) * (v.z - c.z) + (v.w - c.w) * (v.w - c.w);
      nn += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    s_spread += sp; s_norm += nn; cnt += 1.0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s_spread += __shfl_xor(s_spread, o); s_norm += __shfl_xor(s_norm, o); cnt += __shfl_xor(cnt, o);
  }
  if (lane == 0 && cnt > 0.0) { atomicAdd(out, s_spread); atomicAdd(out + 1, s_norm); atomicAdd(out + 2, cnt); }
}

// ------------------------------------------------------------------------------------------
// bf16 x 3 ranking: every stored value x is split as hi + lo with hi = bf16(x), lo = bf16(x - hi)
// (|x - hi| <= 2^-8 |x|, |x - hi - lo| <= 2^-17 |x|); q.v ~ hi.hi + hi.lo + lo.hi on the bf16 matrix pipe (16x the f32 rate)
// ------------------------------------------------------------------------------------------
// f32 blocks [quad][64] float4 -> bf16 blocks [chunk of 16 dims][plane hi/lo][half of 8 dims][64] x 16 B: the
// image a 32x32x16 MFMA wants (lane (j,h) reads the 8 consecutive dims 16c+8h.. of vector j as one ds_read_b128),
// same bytes per block as the f32 form
// (the column of vector v of a block in the image: image_column, slot_filter.hpp)

__global__ void split_bf16_kernel(const float4 *blocks, uint32_t dq, uint64_t nblocks, uint4 *out, const float4 *mu = nullptr) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (block, chunk, half, vector)
  const uint32_t nc = dq / 4;
  if (t >= nblocks * nc * 2 * 64) return;
  const uint32_t v = (uint32_t)(t & 63), h = (uint32_t)((t >> 6) & 1);
  const uint64_t bc = t >> 7;
  const uint32_t c = (uint32_t)(bc % nc);
  const uint64_t b = bc / nc;
  const float4 *src = blocks + (b * dq + 4 * c + 2 * h) * 64 + v;
  uint4 hi, lo;
  float4 v0 = src[0], v1 = src[64];
  if (mu) {  // the image of fl(v - mu)
    const float4 m0 = mu[4 * c + 2 * h], m1 = mu[4 * c + 2 * h + 1];
    v0.x -= m0.x; v0.y -= m0.y; v0.z -= m0.z; v0.w -= m0.w;
    v1.x -= m1.x; v1.y -= m1.y; v1.z -= m1.z; v1.w -= m1.w;
  }
  split8(v0, v1, 1.0f, hi, lo);
  uint4 *dst = out + ((b * nc + c) * 4) * 64;
  const uint32_t col = image_column(v);
  dst[(0 * 2 + h) * 64 + col] = hi;
  dst[(1 * 2 + h) * 64 + col] = lo;
}

// the squared norms in image order (the accumulator of MFMA row i starts at the norm of the vector in column i)
__global__ void image_norms_kernel(const float *xnorm, uint64_t nslots, float *out) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < nslots) out[(s & ~63ull) + image_column((uint32_t)(s & 63u))] = xnorm[s];
}

// bf16-exact stored values: the hi plane IS the value.  A second copy of it in the blocks' own vector order — piece
// (chunk c, half h) of vector v at (block * 2 nc + 2c + h) * 64 + v — lets the select re-evaluate a 16-vector sub-block
// from 256 contiguous bytes per 8 dimensions: half the cache lines of the f32 quads (the MFMA image's column order
// interleaves the two sub-blocks of a tile within every line).
__global__ void hi_natural_kernel(const uint4 *img, uint32_t nc, uint64_t nblocks, uint4 *out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (block, chunk, half, vector)
  if (t >= nblocks * nc * 2 * 64) return;
  const uint32_t v = (uint32_t)(t & 63), h = (uint32_t)((t >> 6) & 1);
  const uint64_t bc = t >> 7;
  const uint32_t c = (uint32_t)(bc % nc);
  const uint64_t b = bc / nc;
  out[((b * nc + c) * 2 + h) * 64 + v] = img[(((b * nc + c) * 4) + h) * 64 + image_column(v)];
}

// The coarse table once more, row-major (centroid c = dim consecutive floats): the coarse select re-evaluates ONE
// centroid per candidate sub-block, and a lone row of a lane-interleaved block is 16 bytes in each of dim / 4 cache
// lines; from this copy it is dim / 32 whole lines.  (k' x dim floats; the lists stay lane-interleaved only.)
__global__ void rows_from_blocks_kernel(const float4 *blocks, uint32_t dq, uint32_t nrows, uint32_t nquad, float4 *out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)nrows * nquad) return;
  const uint32_t row = (uint32_t)(t / nquad), qd = (uint32_t)(t % nquad);
  out[t] = blocks[((size_t)(row / 64) * dq + qd) * 64 + (row % 64)];
}

// 8-bit descriptors (every stored value an integer in 0..255, as SIFT's): one byte per dimension, 16 dimensions of vector
// v at (block * ceil(dq / 4) + p) * 64 + v — a 16-vector sub-block is re-evaluated from 256 contiguous bytes per 16
// dimensions, half of the bf16 copy again.  `not_u8` is raised if some value does not fit.
__global__ void u8_check_kernel(const float4 *blocks, uint64_t nquads, uint32_t *not_u8) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (t < nquads) {
    const float4 v = blocks[t];
    auto ok = [](float x) { return x >= 0.0f && x <= 255.0f && x == floorf(x); };
    bad = !(ok(v.x) && ok(v.y) && ok(v.z) && ok(v.w));
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(not_u8, 1u);
}
__global__ void u8_natural_kernel(const float4 *blocks, uint32_t dq, uint64_t nblocks, uint4 *out) {
  const uint32_t np = (dq + 3) / 4;  // pieces of 16 dimensions (dq is a multiple of 4)
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (block, piece, vector)
  if (t >= nblocks * np * 64) return;
  const uint32_t v = (uint32_t)(t & 63);
  const uint64_t bp = t >> 6;
  const uint32_t p = (uint32_t)(bp % np);
  const uint64_t b = bp / np;
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 x = blocks[(b * dq + 4 * p + i) * 64 + v];
    w[i] = (uint32_t)x.x | ((uint32_t)x.y << 8) | ((uint32_t)x.z << 16) | ((uint32_t)x.w << 24);
  }
  out[t] = make_uint4(w[0], w[1], w[2], w[3]);
}

// 8-bit descriptors ranked with int8 products (rank_stream_i8_kernel), in the frame shifted by 127: the A operand is
// 127 - v (fits in int8 for v in 0..255), 0 on the dimensions past dim.  Same block and column order as the bf16 image
// (image_column): per block nc32 chunks of 32 dimensions x [half of 16 dimensions] x 64 columns x 16 B.
__global__ void i8_image_kernel(const float4 *blocks, uint32_t dq, uint32_t dim, uint32_t nc32, uint64_t nblocks, uint4 *out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (block, chunk, half, vector)
  if (t >= nblocks * nc32 * 2 * 64) return;
  const uint32_t v = (uint32_t)(t & 63), h = (uint32_t)((t >> 6) & 1);
  const uint64_t bc = t >> 7;
  const uint32_t c = (uint32_t)(bc % nc32);
  const uint64_t b = bc / nc32;
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t qd = 8u * c + 4u * h + (uint32_t)i;  // quad of dimensions 4 qd .. 4 qd + 3 (dim is a multiple of 4)
    w[i] = 0u;
    if (4u * qd < dim) {
      const float4 x = blocks[(b * dq + qd) * 64 + v];
      w[i] = ((127u - (uint32_t)x.x) & 0xFFu) | (((127u - (uint32_t)x.y) & 0xFFu) << 8) | (((127u - (uint32_t)x.z) & 0xFFu) << 16) |
             ((127u - (uint32_t)x.w) << 24);
    }
  }
  out[((b * nc32 + c) * 2 + h) * 64 + image_column(v)] = make_uint4(w[0], w[1], w[2], w[3]);
}
// ... and the accumulator's start h(v) = ceil(|v - 127|^2 / 2) in image-column order (pad slots, marked kBig in xnorm:
// kI8PadNorm); *xmax2 = max |v - 127|^2
__global__ void i8_norms_kernel(const float4 *blocks, uint32_t dq, uint32_t dim, uint64_t nslots, const float *xnorm, int *out,
                                uint32_t *xmax2) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  const float4 *p = blocks + (s / kWave) * dq * kWave + (s % kWave);
  int n = 0;
  for (uint32_t qd = 0; 4u * qd < dim; ++qd) {
    const float4 x = p[(size_t)qd * kWave];
    const int a = (int)x.x - 127, b = (int)x.y - 127, c = (int)x.z - 127, d = (int)x.w - 127;
    n += a * a + b * b + c * c + d * d;
  }
  const bool pad = !(xnorm[s] < kBig);
  if (!pad) atomicMax(xmax2, (uint32_t)n);
  out[(s & ~63ull) + image_column((uint32_t)(s & 63u))] = pad ? kI8PadNorm : (n + 1) >> 1;
}

// any nonzero lo half in an image? (pieces of 64 uint4: plane = (piece >> 1) & 1)
__global__ void lo_plane_any_kernel(const uint4 *img, uint64_t npieces, uint32_t *any) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npieces * 64) return;
  const uint64_t piece = t >> 6;
  if (((piece >> 1) & 1) == 0) return;
  const uint4 v = img[t];
  if (((v.x | v.y | v.z | v.w) & 0x7FFF7FFFu) != 0u) atomicOr(any, 1u);
}

// ------------------------------------------------------------------------------------------
// host side: the steps of prepare_rank_images, in the order they run on ix->stream
// ------------------------------------------------------------------------------------------
// a 1-D kernel of 256-thread workgroups over n elements (every argument spelled out: no defaults through a pointer)
template <class... P, class... A>
void launch_1d(hipStream_t st, void (*kernel)(P...), uint64_t n, A... args) {
  hipLaunchKernelGGL(kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, args...);
}

// clear the device word, run `work` (launches and copies on st), read the word back, synchronise
template <class F>
vi_status word_after(hipStream_t st, uint32_t *word, uint32_t *out, F &&work) {
  VI_HIP(hipMemsetAsync(word, 0, 4, st));
  VI_TRY(work());
  VI_HIP(hipGetLastError());
  VI_HIP(hipMemcpyAsync(out, word, 4, hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  return VI_OK;
}
template <class F>
vi_status word_after(hipStream_t st, uint32_t *word, float *out, F &&work) {  // ... the float whose bits it holds
  uint32_t bits = 0;
  VI_TRY(word_after(st, word, &bits, work));
  std::memcpy(out, &bits, 4);
  return VI_OK;
}

const float4 *quads(const BlockSet &s) { return (const float4 *)s.blocks.p; }
uint64_t slots(const BlockSet &s) { return s.nblocks * kWave; }
uint64_t image_threads(const BlockSet &s) { return s.nblocks * (s.dq / 4) * 128; }  // (block, chunk, half, vector) of a bf16 image

// the table's pad slots (>= nlists) must never rank
vi_status mark_table_pads(DeviceIndex *ix, float *norms) {
  const uint64_t npad = slots(ix->centroids) - ix->nlists;
  if (npad) {
    std::vector<float> inf(npad, kBig);
    VI_HIP(hipMemcpyAsync(norms + ix->nlists, inf.data(), npad * 4, hipMemcpyHostToDevice, ix->stream));
  }
  return VI_OK;
}

// xnorm, cent_xnorm, xmax2, cent_xmax2, xnorm_img, cent_xnorm_img: squared norms per slot (kBig on pad slots), their
// maxima, and the same in the column order of the images
vi_status slot_norms(DeviceIndex *ix, uint32_t *word) {
  const hipStream_t st = ix->stream;
  const uint64_t nslots = slots(ix->lists), cslots = slots(ix->centroids);
  VI_TRY(ix->xnorm.reserve(std::max<uint64_t>(1, nslots)));
  VI_TRY(word_after(st, word, &ix->xmax2, [&]() -> vi_status {
    if (!nslots) return VI_OK;
    launch_1d(st, slot_norms_kernel, nslots, quads(ix->lists), ix->dq, nslots, ix->xnorm.p, word, nullptr);
    if (ix->nlists) launch_1d(st, pad_norms_kernel, ix->nlists * 64, ix->list_first_block.p, ix->list_len.p, (uint32_t)ix->nlists, ix->xnorm.p);
    return VI_OK;
  }));
  VI_TRY(ix->cent_xnorm.reserve(std::max<uint64_t>(1, cslots)));
  VI_TRY(word_after(st, word, &ix->cent_xmax2, [&]() -> vi_status {
    if (!cslots) return VI_OK;
    launch_1d(st, slot_norms_kernel, cslots, quads(ix->centroids), ix->dq, cslots, ix->cent_xnorm.p, word, nullptr);
    VI_HIP(hipGetLastError());
    return mark_table_pads(ix, ix->cent_xnorm.p);
  }));
  VI_TRY(ix->xnorm_img.reserve(std::max<uint64_t>(1, nslots)));
  VI_TRY(ix->cent_xnorm_img.reserve(std::max<uint64_t>(1, cslots)));
  if (nslots) launch_1d(st, image_norms_kernel, nslots, ix->xnorm.p, nslots, ix->xnorm_img.p);
  if (cslots) launch_1d(st, image_norms_kernel, cslots, ix->cent_xnorm.p, cslots, ix->cent_xnorm_img.p);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// lists_bf16, cent_bf16 (same size as the f32 blocks), about `mu` if given
vi_status split_images(DeviceIndex *ix, const float4 *mu) {
  const uint64_t nt_l = image_threads(ix->lists), nt_c = image_threads(ix->centroids);
  if (nt_l) launch_1d(ix->stream, split_bf16_kernel, nt_l, quads(ix->lists), ix->dq, ix->lists.nblocks, (uint4 *)ix->lists_bf16.p, mu);
  if (nt_c) launch_1d(ix->stream, split_bf16_kernel, nt_c, quads(ix->centroids), ix->dq, ix->centroids.nblocks, (uint4 *)ix->cent_bf16.p, mu);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// lists_bf16, cent_bf16, lists_lo_zero, cent_lo_zero: the images, and whether every stored value is bf16-exact (8-bit
// descriptors): the lo planes are all zero then and need not be streamed
vi_status bf16_images(DeviceIndex *ix, uint32_t *word) {
  const hipStream_t st = ix->stream;
  const uint64_t per_block = (uint64_t)ix->dq * kWave * 4;  // uint32 words per block
  VI_TRY(ix->lists_bf16.reserve(std::max<uint64_t>(1, ix->lists.nblocks * per_block)));
  VI_TRY(ix->cent_bf16.reserve(std::max<uint64_t>(1, ix->centroids.nblocks * per_block)));
  VI_TRY(split_images(ix, nullptr));
  const uint64_t np_l = ix->lists.nblocks * ix->dq, np_c = ix->centroids.nblocks * ix->dq;
  uint32_t any_l = 0, any_c = 0;
  VI_TRY(word_after(st, word, &any_l, [&]() -> vi_status {
    if (np_l) launch_1d(st, lo_plane_any_kernel, np_l * 64, (const uint4 *)ix->lists_bf16.p, np_l, word);
    return VI_OK;
  }));
  VI_TRY(word_after(st, word, &any_c, [&]() -> vi_status {
    if (np_c) launch_1d(st, lo_plane_any_kernel, np_c * 64, (const uint4 *)ix->cent_bf16.p, np_c, word);
    return VI_OK;
  }));
  ix->lists_lo_zero = np_l > 0 && any_l == 0;
  ix->cent_lo_zero = np_c > 0 && any_c == 0;
  return VI_OK;
}

// what the centring decision weighs: the mean mu (left in ix->centre), the norms about it and their maxima, |mu|^2
struct CentredNorms {
  DevBuf<float> lists, table;  // per slot, kBig on the lists' pad slots
  float xmax2 = 0.0f, cent_xmax2 = 0.0f;
  double mu2 = 0.0;
};
vi_status centred_norms(DeviceIndex *ix, CentredNorms *c) {
  const hipStream_t st = ix->stream;
  const uint64_t nslots = slots(ix->lists), cslots = slots(ix->centroids);
  DevBuf<double> sums;
  VI_TRY(sums.reserve((uint64_t)ix->dq * 4));
  VI_TRY(ix->centre.reserve((uint64_t)ix->dq * 4));
  VI_TRY(c->lists.reserve(nslots));
  VI_TRY(c->table.reserve(cslots));
  VI_HIP(hipMemsetAsync(sums.p, 0, (uint64_t)ix->dq * 4 * sizeof(double), st));
  hipLaunchKernelGGL(mean_kernel, dim3(ix->dq, 64), dim3(256), 0, st, quads(ix->lists), ix->dq, ix->lists.nblocks, sums.p);
  launch_1d(st, mean_finish_kernel, ix->dq * 4, sums.p, ix->dim, ix->dq * 4, (double)ix->nvec_resident, ix->centre.p);
  const float4 *mu = (const float4 *)ix->centre.p;
  uint32_t mxb[2] = {0u, 0u};
  DevBuf<uint32_t> mx2;
  VI_TRY(mx2.reserve(2));
  VI_HIP(hipMemsetAsync(mx2.p, 0, 8, st));
  launch_1d(st, slot_norms_kernel, nslots, quads(ix->lists), ix->dq, nslots, c->lists.p, mx2.p, mu);
  launch_1d(st, slot_norms_kernel, cslots, quads(ix->centroids), ix->dq, (uint64_t)ix->nlists, c->table.p, mx2.p + 1, mu);
  launch_1d(st, pad_norms_kernel, ix->nlists * 64, ix->list_first_block.p, ix->list_len.p, (uint32_t)ix->nlists, c->lists.p);
  VI_HIP(hipMemsetAsync(mx2.p, 0, 8, st));  // (the pad slots' zero vectors entered the kernel's own maximum)
  hipLaunchKernelGGL(max_finite_kernel, dim3(256), dim3(256), 0, st, c->lists.p, nslots, mx2.p);
  hipLaunchKernelGGL(max_finite_kernel, dim3(64), dim3(256), 0, st, c->table.p, (uint64_t)ix->nlists, mx2.p + 1);
  VI_HIP(hipGetLastError());
  VI_HIP(hipMemcpyAsync(mxb, mx2.p, 8, hipMemcpyDeviceToHost, st));
  std::vector<double> hs((size_t)ix->dq * 4);
  VI_HIP(hipMemcpyAsync(hs.data(), sums.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  std::memcpy(&c->xmax2, &mxb[0], 4);
  std::memcpy(&c->cent_xmax2, &mxb[1], 4);
  for (uint32_t e = 0; e < ix->dim; ++e) { const double m = hs[e] / (double)ix->nvec_resident; c->mu2 += m * m; }
  return VI_OK;
}

// the mean squared norm of ALL stored vectors (list_spread_kernel only samples)
vi_status mean_norm2_all(DeviceIndex *ix, double *mean) {
  DevBuf<double> acc;
  VI_TRY(acc.reserve(1));
  VI_HIP(hipMemsetAsync(acc.p, 0, sizeof(double), ix->stream));
  hipLaunchKernelGGL(sum_f32_kernel, dim3(256), dim3(256), 0, ix->stream, ix->xnorm.p, slots(ix->lists), acc.p);
  VI_HIP(hipGetLastError());
  VI_HIP(hipMemcpyAsync(mean, acc.p, sizeof(double), hipMemcpyDeviceToHost, ix->stream));
  VI_HIP(hipStreamSynchronize(ix->stream));
  *mean /= (double)ix->nvec_resident;
  return VI_OK;
}

// centre, centered, mean_norm2_c, xmax2_c, cent_xmax2_c (and, when centred, xnorm_img, cent_xnorm_img, lists_bf16,
// cent_bf16 again, cent_lo_zero): real-valued lists get their images about the mean of the stored vectors when that at
// least halves the norms the margins scale with.  vi_center: VI_CENTER, 1 always, 0 never, else by that rule.
vi_status centre_images(DeviceIndex *ix, int vi_center) {
  const hipStream_t st = ix->stream;
  ix->centered = false;
  if (ix->lists_lo_zero || ix->dim > kNarrowDim || !ix->nlists || !ix->nvec_resident || vi_center == 0) return VI_OK;
  CentredNorms c;
  VI_TRY(centred_norms(ix, &c));
  double mean_raw = 0.0;
  VI_TRY(mean_norm2_all(ix, &mean_raw));
  const double mean_c = std::max(0.0, mean_raw - c.mu2);  // the mean of |v - mu|^2 is the mean of |v|^2 less |mu|^2
  const bool gain = mean_c + 2.0 * (double)c.xmax2 < 0.5 * (mean_raw + 2.0 * (double)ix->xmax2);
  if (vi_center != 1 && !gain) return VI_OK;
  ix->centered = true;
  ix->mean_norm2_c = (float)mean_c;
  ix->xmax2_c = c.xmax2;
  ix->cent_xmax2_c = c.cent_xmax2;
  const uint64_t nslots = slots(ix->lists), cslots = slots(ix->centroids);
  if (cslots - ix->nlists) {
    VI_TRY(mark_table_pads(ix, c.table.p));
    VI_HIP(hipStreamSynchronize(st));
  }
  launch_1d(st, image_norms_kernel, nslots, c.lists.p, nslots, ix->xnorm_img.p);
  launch_1d(st, image_norms_kernel, cslots, c.table.p, cslots, ix->cent_xnorm_img.p);
  VI_TRY(split_images(ix, (const float4 *)ix->centre.p));
  VI_HIP(hipStreamSynchronize(st));
  ix->cent_lo_zero = false;
  return VI_OK;
}

// rho2_max: what the hi planes of real-valued lists leave out (rank_approx_mode)
vi_status hi_plane_residual(DeviceIndex *ix, uint32_t *word) {
  const uint64_t nslots = slots(ix->lists);
  ix->rho2_max = 0.0f;
  if (ix->lists_lo_zero || ix->dim > kNarrowDim || !nslots) return VI_OK;
  return word_after(ix->stream, word, &ix->rho2_max, [&]() -> vi_status {
    launch_1d(ix->stream, trunc_residual_kernel, nslots, quads(ix->lists), ix->dq, nslots, ix->xnorm.p,
              ix->centered ? (const float4 *)ix->centre.p : nullptr, word);
    return VI_OK;
  });
}

// cent_rows: single-row exact re-evaluation of the coarse select
vi_status coarse_rows(DeviceIndex *ix) {
  if (!ix->nlists || ix->dim > kNarrowDim) return VI_OK;
  const uint32_t nquad = ix->dim / 4;
  VI_TRY(ix->cent_rows.reserve((uint64_t)ix->nlists * ix->dim));
  launch_1d(ix->stream, rows_from_blocks_kernel, (uint64_t)ix->nlists * nquad, quads(ix->centroids), ix->dq, (uint32_t)ix->nlists, nquad,
            (float4 *)ix->cent_rows.p);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// mean_spread, mean_norm2: how far the vectors of real-valued lists sit from their centroids (cent_rows), against how
// large they are (rank_approx_mode)
vi_status list_spread(DeviceIndex *ix) {
  if (!ix->nlists || ix->dim > kNarrowDim || !ix->lists.nblocks || ix->lists_lo_zero) return VI_OK;
  DevBuf<double> sums;
  VI_TRY(sums.reserve(3));
  VI_HIP(hipMemsetAsync(sums.p, 0, 3 * sizeof(double), ix->stream));
  hipLaunchKernelGGL(list_spread_kernel, dim3((uint32_t)ix->nlists), dim3(64), 0, ix->stream, quads(ix->lists), ix->dq,
                     (const float4 *)ix->cent_rows.p, ix->dim, ix->list_first_block.p, ix->list_len.p, (uint32_t)ix->nlists, 8u, sums.p);
  VI_HIP(hipGetLastError());
  double h[3] = {0, 0, 0};
  VI_HIP(hipMemcpyAsync(h, sums.p, sizeof(h), hipMemcpyDeviceToHost, ix->stream));
  VI_HIP(hipStreamSynchronize(ix->stream));
  if (h[2] > 0) { ix->mean_spread = (float)(h[0] / h[2]); ix->mean_norm2 = (float)(h[1] / h[2]); }
  return VI_OK;
}

// lists_u8_nat, lists_i8, i8_norm_img, i8_centre, i8_xmax2: bf16-exact lists that are 8-bit descriptors get their byte
// copy, and the int8 image and norms of the streaming rank kernel's int8 form (rank_stream_i8_kernel) with the frame's
// centre (127 on every dimension) for the select's margins
vi_status u8_images(DeviceIndex *ix, uint32_t *word) {
  const hipStream_t st = ix->stream;
  if (!ix->lists_lo_zero || ix->dim > kNarrowDim || !ix->lists.nblocks) return VI_OK;  // (bf16-exact is necessary)
  const uint64_t nslots = slots(ix->lists), nquads = ix->lists.nblocks * ix->dq * 64;
  uint32_t not_u8 = 1;
  VI_TRY(word_after(st, word, &not_u8, [&]() -> vi_status {
    launch_1d(st, u8_check_kernel, nquads, quads(ix->lists), nquads, word);
    return VI_OK;
  }));
  if (not_u8) return VI_OK;
  const uint64_t nt8 = ix->lists.nblocks * (ix->dq / 4) * 64;
  VI_TRY(ix->lists_u8_nat.reserve(nt8 * 4));
  launch_1d(st, u8_natural_kernel, nt8, quads(ix->lists), ix->dq, ix->lists.nblocks, (uint4 *)ix->lists_u8_nat.p);
  VI_HIP(hipGetLastError());
  const uint32_t nc32 = (ix->dim + 31) / 32;
  const uint64_t nti = ix->lists.nblocks * nc32 * 128;
  VI_TRY(ix->lists_i8.reserve(nti * 4));
  VI_TRY(ix->i8_norm_img.reserve(nslots));
  VI_TRY(ix->i8_centre.reserve(ix->dim));
  const std::vector<float> c127(ix->dim, 127.0f);  // (read by the copy below until word_after's synchronise)
  uint32_t n2 = 0;
  VI_TRY(word_after(st, word, &n2, [&]() -> vi_status {
    launch_1d(st, i8_image_kernel, nti, quads(ix->lists), ix->dq, ix->dim, nc32, ix->lists.nblocks, (uint4 *)ix->lists_i8.p);
    launch_1d(st, i8_norms_kernel, nslots, quads(ix->lists), ix->dq, ix->dim, nslots, ix->xnorm.p, ix->i8_norm_img.p, word);
    VI_HIP(hipGetLastError());
    VI_HIP(hipMemcpyAsync(ix->i8_centre.p, c127.data(), ix->dim * sizeof(float), hipMemcpyHostToDevice, st));
    return VI_OK;
  }));
  ix->i8_xmax2 = (float)n2;
  return VI_OK;
}

// lists_hi_nat: exact re-evaluation of bf16-exact lists from bf16 (select_kernel), where no byte copy serves
vi_status hi_natural(DeviceIndex *ix) {
  if (!ix->lists_lo_zero || ix->dim > kNarrowDim || ix->lists_u8_nat.p) return VI_OK;
  VI_TRY(ix->lists_hi_nat.reserve(ix->lists.nblocks * (uint64_t)ix->dq * kWave * 4 / 2));
  launch_1d(ix->stream, hi_natural_kernel, image_threads(ix->lists), (const uint4 *)ix->lists_bf16.p, ix->dq / 4, ix->lists.nblocks,
            (uint4 *)ix->lists_hi_nat.p);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// c_first, c_len: the coarse table described as one list
vi_status table_as_one_list(DeviceIndex *ix) {
  const uint32_t one_first[1] = {0u}, one_len[1] = {(uint32_t)ix->nlists};
  VI_TRY(ix->c_first.reserve(1));
  VI_TRY(ix->c_len.reserve(1));
  VI_HIP(hipMemcpy(ix->c_first.p, one_first, 4, hipMemcpyHostToDevice));
  VI_HIP(hipMemcpy(ix->c_len.p, one_len, 4, hipMemcpyHostToDevice));
  return VI_OK;
}

}  // namespace

vi_status prepare_rank_images(DeviceIndex *ix) {
  const char *ce = getenv("VI_CENTER");  // a load-time option: '0' never, '1' always, else by the halving rule
  const int vi_center = ce && *ce == '0' ? 0 : ce && *ce == '1' ? 1 : -1;
  DevBuf<uint32_t> word;  // the device word the steps' maxima and flags come back through
  VI_TRY(word.reserve(1));
  VI_TRY(slot_norms(ix, word.p));
  if ((ix->dim & 3) == 0 && ix->dim <= kMaxMfmaDim) {  // (otherwise the MFMA engine never runs: no images)
    VI_TRY(bf16_images(ix, word.p));
    VI_TRY(centre_images(ix, vi_center));
    VI_TRY(hi_plane_residual(ix, word.p));
    VI_TRY(coarse_rows(ix));
    VI_TRY(list_spread(ix));
    VI_TRY(u8_images(ix, word.p));
    VI_TRY(hi_natural(ix));
  }
  return table_as_one_list(ix);
}

}  // namespace vi
