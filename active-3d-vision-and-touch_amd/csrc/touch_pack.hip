// touch_pack.hip — the outputs of a3vt_touch_render / a3vt_touch_finish for I views in the form a data set stores them: the touch
// images as uint8, and the views' contact clouds packed end to end behind an offsets table.  What a host read then moves is what it
// keeps: a padded points buffer is 14 641 rows (176 KB) per view whatever the view's count, and a float image four times its file.
//
// ONE launch with two kinds of workgroup, told apart by blockIdx.x alone.
//
// * Cloud groups, `spans * chunks` of them.  Group (g, c) owns the views [g * span, (g + 1) * span) and, of each view's 3 n_i dwords,
//   the dwords [c * chunk_len, (c + 1) * chunk_len).  It needs the exclusive prefix at its first view and the total, and takes both
//   straight from count / status: every thread sums n_j over a strided share of ALL I views into two integers, (j < first) and all,
//   then a butterfly per wave and four LDS words per sum.  Integer sums: any order gives the same value, so the result does not
//   depend on span, chunks or the grid.  No workgroup reads what another wrote — no atomics, no fence, no second launch; the price
//   is that each cloud group reads the 8 I bytes of count and status again, from L2 (at I = 65 536 that is 512 KB for each of 2 048
//   groups, against 11.5 GB of images in the same launch; at I = 1 600 it is 12.8 KB).  The span's own prefixes come from a serial
//   walk over at most kPackMaxSpan values in LDS.  Then the copy: dwords with consecutive addresses, thread after thread.  A cloud
//   row is 12 bytes and the offsets are arbitrary, so source and destination agree on a 16-byte phase for one view in four only;
//   the copy is dword-granular like touch_assemble's.  Values move as uint32_t: NaN payloads and -0 are bits like any other.
//   Chunk 0 of a span writes the span's offsets; the group of the last span also writes offsets[I].  When the total exceeds
//   `capacity` every group still writes its offsets and none writes a cloud row.
// * Image groups, the rest of the grid: the I * 121 * 121 * 3 floats as ONE flat array (a view is 175 692 bytes, no multiple of 16,
//   so only the base is aligned), a 16-byte load and a 4-byte store per lane and step, four steps in flight, grid-stride; the last
//   0..3 floats by scalar moves.  clamp-then-truncate is two compares and selects that send NaN (and -0) to 0, then v_cvt_u32_f32.
//
// n_i is count[i] clamped into 0..14 641 where status[i] == 1, else 0: a count the renderer cannot produce neither reads outside
// points[i] nor breaks the capacity rule.  No input is written.
#include "common.h"
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {

constexpr int kPackThreads = 256;
constexpr int kPackWaves = kPackThreads / kWave;
constexpr int kPackPixels = kTouchRes * kTouchRes;           // 14 641: the rows of a view's points
constexpr int kPackViewDwords = kPackPixels * 3;             // 43 923: a view's points, and a view's image
constexpr int kPackMaxSpan = 64;                             // views of one cloud group (kTouchMaxImages / kPackMaxSpan spans at most)
constexpr int kPackTargetGroups = 2048;                      // cloud groups wanted before a view is split no further
constexpr int kPackMaxChunks = 16;
constexpr int kPackImageGroups = 4096;                       // image groups at most: 16 waves a CU, the rest by stride
constexpr int kPackUnroll = 4;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int pack_rows(const int32_t *__restrict__ count, const int32_t *__restrict__ status, int j) {
  return status[j] == 1 ? min(max(count[j], 0), kPackPixels) : 0;
}

__device__ __forceinline__ uint32_t pack_u8(float v) {       // clamp to [0, 255], then toward zero; NaN and -0 give 0
  const float low = v > 0.f ? v : 0.f;
  return (uint32_t)(low < 255.f ? low : 255.f);
}

__device__ __forceinline__ uint32_t pack_u8x4(f32x4 v) {
  return pack_u8(v[0]) | (pack_u8(v[1]) << 8) | (pack_u8(v[2]) << 16) | (pack_u8(v[3]) << 24);
}

__global__ __launch_bounds__(kPackThreads) void touch_pack_kernel(const float *__restrict__ touch, const uint32_t *__restrict__ points,
                                                                  const int32_t *__restrict__ count, const int32_t *__restrict__ status,
                                                                  int I, int capacity, int span, int chunks, int chunk_len, int cloud_groups,
                                                                  uint8_t *__restrict__ touch_u8, int32_t *__restrict__ offsets,
                                                                  uint32_t *__restrict__ cloud) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= cloud_groups) {                     // ---- an image group (uniform per workgroup)
    const long long total = (long long)I * kPackViewDwords, quads = total >> 2;
    const long long stride = (long long)(gridDim.x - cloud_groups) * kPackThreads;
    const f32x4 *__restrict__ src = reinterpret_cast<const f32x4 *>(touch);
    uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(touch_u8);
    long long q = (long long)((int)blockIdx.x - cloud_groups) * kPackThreads + tid;
    for (; q + (kPackUnroll - 1) * stride < quads; q += kPackUnroll * stride) {
      f32x4 v[kPackUnroll];
#pragma unroll
      for (int u = 0; u < kPackUnroll; ++u) v[u] = __builtin_nontemporal_load(src + q + u * stride);
#pragma unroll
      for (int u = 0; u < kPackUnroll; ++u) dst[q + u * stride] = pack_u8x4(v[u]);
    }
    for (; q < quads; q += stride) dst[q] = pack_u8x4(__builtin_nontemporal_load(src + q));
    if ((int)blockIdx.x == cloud_groups && tid < (int)(total & 3)) touch_u8[(quads << 2) + tid] = (uint8_t)pack_u8(touch[(quads << 2) + tid]);
    return;
  }

  // ---- a cloud group
  __shared__ int s_part[2][kPackWaves];
  __shared__ int s_rows[kPackMaxSpan];
  const int g = (int)blockIdx.x / chunks, c = (int)blockIdx.x % chunks;
  const int first = g * span, last = min(first + span, I);   // (first < I: the host launches cdiv(I, span) spans)
  int before = 0, all = 0;
  for (int j = tid; j < I; j += kPackThreads) {
    const int n = pack_rows(count, status, j);
    all += n;
    before += j < first ? n : 0;
  }
  before = wave_sum_int(before);
  all = wave_sum_int(all);
  if ((tid & (kWave - 1)) == 0) {
    s_part[0][tid / kWave] = before;
    s_part[1][tid / kWave] = all;
  }
  if (tid < last - first) s_rows[tid] = pack_rows(count, status, first + tid);   // (span <= kPackMaxSpan <= kPackThreads)
  __syncthreads();
  before = all = 0;
#pragma unroll
  for (int w = 0; w < kPackWaves; ++w) {
    before += s_part[0][w];
    all += s_part[1][w];
  }
  if (c == 0) {
    if (tid == 0) {
      int at = before;
      for (int i = first; i < last; ++i) {
        offsets[i] = at;
        at += s_rows[i - first];
      }
      if (last == I) offsets[I] = at;
    }
  }
  if (all > capacity) return;                                // (uniform over the whole launch: no row of cloud is written)
  const int lo = c * chunk_len;
  long long at = before;                                     // rows before view i
  for (int i = first; i < last; ++i) {
    const int rows = s_rows[i - first];
    const int hi = min(lo + chunk_len, rows * 3);
    const uint32_t *__restrict__ src = points + (long long)i * kPackViewDwords;
    uint32_t *__restrict__ dst = cloud + at * 3;
    for (int k = lo + tid; k < hi; k += kPackThreads) dst[k] = src[k];
    at += rows;
  }
}

}  // namespace

int launch_touch_pack(const float *touch, const float *points, const int32_t *count, const int32_t *status, int I, int capacity,
                      uint8_t *touch_u8, int32_t *offsets, float *cloud, hipStream_t s) {
  int span = 1, chunks = 1, chunk_len = kPackViewDwords, cloud_groups = 0;
  if (points) {
    span = cdiv(I, kPackTargetGroups);                       // 1 up to 2 048 views, 32 at kTouchMaxImages
    if (span > kPackMaxSpan) span = kPackMaxSpan;
    const int spans = cdiv(I, span);
    chunks = kPackTargetGroups / spans;
    chunks = chunks < 1 ? 1 : chunks > kPackMaxChunks ? kPackMaxChunks : chunks;
    chunk_len = cdiv(kPackViewDwords, chunks);
    cloud_groups = spans * chunks;
  }
  int image_groups = 0;
  if (touch) {
    const long long quads = ((long long)I * kPackViewDwords) >> 2;
    const long long want = (quads + kPackThreads - 1) / kPackThreads;
    image_groups = (int)(want < 1 ? 1 : want > kPackImageGroups ? kPackImageGroups : want);
  }
  A3VT_LAUNCH(touch_pack_kernel, dim3(cloud_groups + image_groups), dim3(kPackThreads), 0, s, touch,
              reinterpret_cast<const uint32_t *>(points), count, status, I, capacity, span, chunks, chunk_len, cloud_groups, touch_u8, offsets,
              reinterpret_cast<uint32_t *>(cloud));
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
