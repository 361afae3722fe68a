// chart_head.hip — the tail of the touch chart predictor (reconstruction/touch/model.py: Encoder.fc, the template add and
// transform_verts) and the slot rule of policies/scoring.py:touch_slots, in ONE launch: from the 512 features of n views to the
// (n, 25, 4) rows of touch_charts.npy — x, y, z, mask — and, on request, the charts / masks tensors touch_slots returns.
//
// Shape.  A workgroup takes a tile of kHeadRows = 16 views: the M of v_mfma_f32_16x16x4_f32.  Its activations stay in LDS (16 x 512
// features, then 16 x 256, 16 x 128, 16 x 75); the weights stream from L2 in torch's own [out][in] layout (W1 alone is 512 KB, so
// nothing of them is staged: a lane's 16-byte load of a weight row IS its B operand).  Eight waves: a wave owns 16 output columns
// of a layer at a time (layer 1: two such tiles per wave, layer 2: one, layer 3: five of the eight waves).
//
// Why the matrix pipe.  Exact fp32 either way (the MFMA is a k-ordered fmaf chain, the same numerics as v_fma_f32 at the same peak
// rate), but the MFMA wants ONE register per operand and lane where a VALU formulation of a 16-row tile keeps 16 activations per
// weight in registers or re-reads LDS per multiply-add, and it leaves the VALU idle for the address arithmetic.  The kernel is
// latency-bound (n = 600 is 38 workgroups), so what counts is the length of a wave's dependent chain: see "order" below.
//
// Order of every sum (fixed: it depends on neither n nor the row's place in the batch, so the results are bit-repeatable and
// batch-invariant).  Output (row i, column j) of a layer with K inputs: the K inputs are cut into blocks of 16; block b goes to
// accumulator b % C, C = min(16, K / 16); inside a block the MFMA step t = 0..3 adds the products of k = 16 b + 4 g + t for
// g = 0, 1, 2, 3 in that order onto the accumulator; the C accumulators are added as a pairwise tree (q takes q + C / 2, then
// q + C / 4, ...), then + bias.  Sixteen chains of at most 32 terms instead of one of 512: the dependent latency of a tile is that of
// its longest chain, and the rounding error of a sum grows with the length of its chains (a running fp32 sum rounds at every step
// by half an ulp of the partial sum; a tree of short chains keeps the count of roundings a term passes through at 32 + 4).  A row
// of the tile never meets another row's values (the MFMA's row i reads row i of A only), so a NaN stays in its row.
//
// The slot rule is a SELECT on the row's code (2: the transformed chart, mask 2; 1: the finger's position 25 times, mask 1; anything
// else: zeros, mask 0): a NaN in the features, the rotation or — for code 0 — the position of a row whose code is not 2 does not
// reach its output.  Rows beyond n in the last tile compute on zeros and write nothing.
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {

constexpr int kHeadThreads = 512, kHeadWaves = kHeadThreads / kWave;
constexpr int kHeadChains = 16;   // independent accumulators of a tile (K = 512: 32 terms each, 256: 16, 128: 8 chains of 16)
constexpr int kHeadPad = 4;   // floats added to an LDS row: the 16 rows of a ds_read_b128 fall on 16 different 16-byte slots

// Rows j0 .. j0 + 15 of w ([n_out][K], torch's layout) times the tile's 16 activation rows x (LDS, ldx floats apart): the 16 x 16
// block D[i][j0 + (lane & 15)], i = 4 (lane >> 4) + reg — the order of the sums is the file header's.
template <int K>
__device__ __forceinline__ f32x4 head_tile(const float *__restrict__ w, int n_out, int j0, const float *x, int ldx, int lane) {
  const int r = lane & 15, g = lane >> 4, j = j0 + r;
  const bool live = j < n_out;                                   // (layer 3: 75 rows, the fifth tile has 11)
  const float *__restrict__ wrow = w + (size_t)(live ? j : 0) * K + 4 * g;
  const float *xrow = x + r * ldx + 4 * g;
  constexpr int kAcc = K / 16 < kHeadChains ? K / 16 : kHeadChains;
  f32x4 acc[kAcc] = {};
#pragma unroll
  for (int b = 0; b < K / 16; b += kAcc) {
#pragma unroll
    for (int q = 0; q < kAcc; ++q) {
      f32x4 wv = *reinterpret_cast<const f32x4 *>(wrow + (b + q) * 16);
      if (!live) wv = (f32x4){0.f, 0.f, 0.f, 0.f};
      const f32x4 xv = *reinterpret_cast<const f32x4 *>(xrow + (b + q) * 16);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[t], wv[t], acc[q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int half = kAcc / 2; half > 0; half /= 2) {   // the pairwise tree: chain q takes chain q + half
#pragma unroll
    for (int q = 0; q < half; ++q) acc[q] = acc[q] + acc[q + half];
  }
  return acc[0];
}

// One Linear of the tile: y[i][j] = act(sum + bias[j]) (+ add[j]: the template, layer 3 only), the waves striding over the column tiles.
template <int K, bool RELU>
__device__ __forceinline__ void head_layer(const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ add,
                                           int n_out, const float *x, int ldx, float *y, int ldy) {
  const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  for (int j0 = wave * 16; j0 < n_out; j0 += kHeadWaves * 16) {   // (uniform per wave)
    const f32x4 d = head_tile<K>(w, n_out, j0, x, ldx, lane);
    const int j = j0 + (lane & 15), i0 = 4 * (lane >> 4);
    if (j >= n_out) continue;
    const float b = bias[j], a = add ? add[j] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float z = __fadd_rn(d[reg], b);
      if (RELU) z = relu_nan(z);
      if (add) z = __fadd_rn(a, z);
      y[(i0 + reg) * ldy + j] = z;
    }
  }
}

__global__ __launch_bounds__(kHeadThreads) void chart_head_kernel(const float *__restrict__ features, const float *__restrict__ w1,
                                                                  const float *__restrict__ b1, const float *__restrict__ w2,
                                                                  const float *__restrict__ b2, const float *__restrict__ w3,
                                                                  const float *__restrict__ b3, const float *__restrict__ tmpl,
                                                                  const float *__restrict__ rot, const float *__restrict__ pos,
                                                                  const int32_t *__restrict__ code, int n, float *__restrict__ rows,
                                                                  float *__restrict__ charts, float *__restrict__ masks) {
  constexpr int ld0 = kHeadIn + kHeadPad, ld1 = kHeadHidden1 + kHeadPad, ld2 = kHeadHidden2 + kHeadPad, ld3 = kHeadOut + 1;
  __shared__ __attribute__((aligned(16))) float x0[kHeadRows * ld0];
  __shared__ __attribute__((aligned(16))) float x1[kHeadRows * ld1];
  __shared__ __attribute__((aligned(16))) float x2[kHeadRows * ld2];
  __shared__ float v[kHeadRows * ld3];
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * kHeadRows;
  for (int idx = tid; idx < kHeadRows * (kHeadIn / 4); idx += kHeadThreads) {
    const int i = idx / (kHeadIn / 4), c = 4 * (idx % (kHeadIn / 4));
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (row0 + i < n) val = *reinterpret_cast<const f32x4 *>(features + (size_t)(row0 + i) * kHeadIn + c);
    *reinterpret_cast<f32x4 *>(x0 + i * ld0 + c) = val;
  }
  __syncthreads();
  head_layer<kHeadIn, true>(w1, b1, nullptr, kHeadHidden1, x0, ld0, x1, ld1);
  __syncthreads();
  head_layer<kHeadHidden1, true>(w2, b2, nullptr, kHeadHidden2, x1, ld1, x2, ld2);
  __syncthreads();
  head_layer<kHeadHidden2, false>(w3, b3, tmpl, kHeadOut, x2, ld2, v, ld3);   // v = template + fc(features)
  __syncthreads();
  for (int idx = tid; idx < kHeadRows * kHeadVerts; idx += kHeadThreads) {
    const int i = idx / kHeadVerts, p = idx % kHeadVerts;
    const long long row = row0 + i;
    if (row >= n) continue;
    const int c = code[row];
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    if (c == 2 || c == 1) {
      const float *__restrict__ P = pos + row * 3;
      if (c == 2) {   // rot . v + pos: the row-times-column sums of bmm, then the add
        const float *__restrict__ R = rot + row * 9;
        const float a = v[i * ld3 + 3 * p], b = v[i * ld3 + 3 * p + 1], d = v[i * ld3 + 3 * p + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
          out[k] = __fadd_rn(__fmaf_rn(R[3 * k + 2], d, __fmaf_rn(R[3 * k + 1], b, __fmul_rn(R[3 * k], a))), P[k]);
        out[3] = 2.f;
      } else {
        out = (f32x4){P[0], P[1], P[2], 1.f};
      }
    }
    const long long at = row * kHeadVerts + p;
    *reinterpret_cast<f32x4 *>(rows + at * 4) = out;
    if (charts) {
      charts[at * 3] = out[0];
      charts[at * 3 + 1] = out[1];
      charts[at * 3 + 2] = out[2];
      masks[at] = out[3];
    }
  }
}

}  // namespace

int launch_touch_chart_head(const float *features, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                            const float *b3, const float *tmpl, const float *rot, const float *pos, const int32_t *code, int n, float *rows,
                            float *charts, float *masks, hipStream_t s) {
  A3VT_LAUNCH(chart_head_kernel, dim3(cdiv(n, kHeadRows)), dim3(kHeadThreads), 0, s, features, w1, b1, w2, b2, w3, b3, tmpl, rot, pos, code,
              n, rows, charts, masks);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
