// qnet_input.hip — the DDQN graph model's per-vertex features and the product of its layer 0, without the feature rows.
//
// Reference: Graph_Model.forward, pterotactyl/policies/DDQN/model.py:100-118.  Layer 0 multiplies the (B N) x 300 rows
// [action embedding a_b | PE(p) | E[token]] by W0 = [Wa; Wp; Wm].  PE = L3(relu(L2(relu(L1(nerf(p) ++ p))))) (63 -> 25 -> 50 ->
// 100) has no activation after L3, so
//   Z0[b, v, :] = S[b, :] + T[token(b, v), :] + relu2(b, v, :) C,     S = a Wa + b3 Wp,  T = E Wm,  C = W3^T Wp
// with the composites S (B x h), T (4 x h), C (50 x h) formed by the caller (torch; autograd carries their gradients on to the
// action model, the embedding table, L3 and the three row blocks of W0).  A row therefore costs the nerf embedding, L1, L2 and a
// 50-term product per output column instead of a 300-term one, and neither the 60 / 63 / 25 / 50 / 100 / 300 wide intermediates
// nor their gradients exist in memory.
//
// Forward: a workgroup takes 64 vertex rows of ONE sample (a sample's rows never depend on the batch around it): the encoder
// runs in LDS, then each wave forms 16 rows x h outputs by plain fp32 FMAs, k ascending (exact fp32; no bf16 operand anywhere).
// Columns [0, pad4(cut_len)) leave raw (the neighbour aggregation adds the bias and the ReLU), the rest leave activated —
// what EPI_FWD_HIDDEN does for the lone layer (a3vt_gcn_layer_fwd).
// Backward: from dZ (after the activation mask and the A^T gather) a workgroup re-runs the encoder for its tiles, forms
// dh2 = dZ C^T, walks back through L2 and L1, and keeps dC, the per-token column sums of dZ (dT; dS is their sum over tokens per
// sample), dW2, db2, dW1, db1 in registers over ALL its tiles; one partial image per workgroup, summed by one launch in a fixed
// order.  No atomics: two calls give the same bits.  No position gradient (observations need none).
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {


constexpr int kRows = 64;                  // vertex rows per tile
constexpr int kE = 63, kH1 = 25, kH2 = 50; // widths of the encoder's input and two hidden activations
constexpr int kLdE = 64, kLdH1 = 28, kLdH2 = 52;   // LDS row strides (pad entries are zero)
constexpr int kKGroup = 13;                // backward: wave g owns rows [13 g, 13 g + 13) of dC (4 x 13 = 52 >= 50)
constexpr int kBwdWgs = 256;
constexpr double kPi = 3.14159265358979323846;
// the reference's ten frequencies (vision/model.py:383-389), each rounded to fp32 once as torch rounds the python scalars
__device__ const float kFreq[10] = {(float)kPi,           (float)(kPi * 2 * 1), (float)(kPi * 2 * 2), (float)(kPi * 2 * 3),
                                    (float)(kPi * 2 * 4), (float)(kPi * 2 * 5), (float)(kPi * 2 * 6), (float)(kPi * 2 * 7),
                                    (float)(kPi * 2 * 8), (float)(kPi * 2 * 9)};

struct EncLds {
  float *e, *h1, *h2, *w1, *b1, *w2, *b2;
  int *tok;
};
constexpr int kEncFloats = kRows * kLdE + kRows * kLdH1 + kRows * kLdH2 + kH1 * kE + 29 + kH2 * kH1 + 2 + 52 + kRows;
static_assert(kEncFloats % 4 == 0 && (kRows * kLdE + kRows * kLdH1) % 4 == 0, "h2 and what follows the block are read 16 bytes at a time");
__device__ __forceinline__ EncLds enc_carve(float *base) {
  EncLds L;
  L.e = base;
  L.h1 = L.e + kRows * kLdE;
  L.h2 = L.h1 + kRows * kLdH1;
  L.w1 = L.h2 + kRows * kLdH2;
  L.b1 = L.w1 + kH1 * kE;
  L.w2 = L.b1 + 29;            // (25 biases; 29 makes the block a multiple of 4 floats)
  L.b2 = L.w2 + kH2 * kH1 + 2;
  L.tok = reinterpret_cast<int *>(L.b2 + 52);
  return L;
}

__device__ __forceinline__ void enc_load_weights(const EncLds &L, const QnetArgs &a) {
  for (int i = threadIdx.x; i < kH1 * kE; i += 256) L.w1[i] = a.w1[i];
  for (int i = threadIdx.x; i < kH2 * kH1; i += 256) L.w2[i] = a.w2[i];
  if (threadIdx.x < kH1) L.b1[threadIdx.x] = a.b1[threadIdx.x];
  if (threadIdx.x < kH2) L.b2[threadIdx.x] = a.b2[threadIdx.x];
}

// e = [sin(f0 p), cos(f0 p), sin(f1 p), ... | p] (index f * 6 + {0: sin, 3: cos} + axis, as torch.stack(..., dim=2) lays it out),
// h1 = relu(W1 e + b1), h2 = relu(W2 h1 + b2) for rows [v0, v0 + nrows) of one sample; rows past nrows run on p = 0.
// Ends with a barrier; the caller puts one between the last reader of the previous tile and this call.
__device__ __forceinline__ void enc_tile(const EncLds &L, const float *__restrict__ mesh_b, int v0, int nrows) {
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kRows * 30; idx += 256) {
    const int row = idx / 30, q = idx - row * 30, f = q / 3, ax = q - f * 3;
    const float p = row < nrows ? mesh_b[(size_t)(v0 + row) * 4 + ax] : 0.f;
    const float ang = p * kFreq[f];
    L.e[row * kLdE + f * 6 + ax] = sinf(ang);
    L.e[row * kLdE + f * 6 + 3 + ax] = cosf(ang);
  }
  {
    const int row = tid >> 2, ax = tid & 3;   // 64 rows x 4 floats = 256 threads
    const float p = row < nrows ? mesh_b[(size_t)(v0 + row) * 4 + ax] : 0.f;
    if (ax < 3) {
      L.e[row * kLdE + 60 + ax] = p;
    } else {
      const int t = (int)p;
      L.tok[row] = t < 0 ? 0 : (t > 3 ? 3 : t);
      L.e[row * kLdE + 63] = 0.f;
    }
  }
  __syncthreads();
  for (int o = tid; o < kRows * kLdH1; o += 256) {
    const int row = o / kLdH1, i = o - row * kLdH1;
    float acc = 0.f;
    if (i < kH1) {
      acc = L.b1[i];
      const float *w = L.w1 + i * kE, *e = L.e + row * kLdE;
#pragma unroll 9
      for (int c = 0; c < kE; ++c) acc = fmaf(w[c], e[c], acc);
      acc = relu_nan(acc);
    }
    L.h1[o] = acc;
  }
  __syncthreads();
  for (int o = tid; o < kRows * kLdH2; o += 256) {
    const int row = o / kLdH2, k = o - row * kLdH2;
    float acc = 0.f;
    if (k < kH2) {
      acc = L.b2[k];
      const float *w = L.w2 + k * kH1, *h = L.h1 + row * kLdH1;
#pragma unroll 5
      for (int i = 0; i < kH1; ++i) acc = fmaf(w[i], h[i], acc);
      acc = relu_nan(acc);
    }
    L.h2[o] = acc;
  }
  __syncthreads();
}

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <bool WIDE>   // WIDE: more than 64 column quads (h > 256): a lane owns quads `lane` and `lane + 64`
__global__ __launch_bounds__(256) void qnet_fwd_kernel(QnetArgs a, int tiles_per) {
  __shared__ __attribute__((aligned(16))) float lds[kEncFloats];
  const EncLds L = enc_carve(lds);
  const int b = blockIdx.x / tiles_per, v0 = (blockIdx.x - b * tiles_per) * kRows;
  const int nrows = a.n_vert - v0 < kRows ? a.n_vert - v0 : kRows;
  const int npad = pad4(a.hidden), nq = npad / 4, cpad = pad4(a.cut_len);
  enc_load_weights(L, a);
  enc_tile(L, a.mesh + (size_t)b * a.n_vert * 4, v0, nrows);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool on0 = lane < nq, on1 = WIDE && lane + 64 < nq;
  const float *__restrict__ C = a.comp_c;
  const bool yvec = (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;
  for (int pass = 0; pass < 2; ++pass) {
    const int r0 = wave * 16 + pass * 8;
    if (r0 >= nrows) break;
    f32x4 acc0[8], acc1[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc0[r] = acc1[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k4 = 0; k4 < kLdH2 / 4; ++k4) {
      f32x4 hv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) hv[r] = ld4(L.h2 + (r0 + r) * kLdH2 + k4 * 4);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int k = k4 * 4 + kk;
        if (k >= kH2) break;
        const f32x4 c0 = on0 ? ld4(C + (size_t)k * npad + lane * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 c1 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (on1) c1 = ld4(C + (size_t)k * npad + (lane + 64) * 4);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          acc0[r] += hv[r][kk] * c0;
          if (WIDE) acc1[r] += hv[r][kk] * c1;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int row = r0 + r;
      if (row >= nrows) break;
      const size_t gr = (size_t)b * a.n_vert + v0 + row;
      const int tk = L.tok[row];
#pragma unroll
      for (int half = 0; half < (WIDE ? 2 : 1); ++half) {
        if (!(half ? on1 : on0)) continue;
        const int col = (lane + 64 * half) * 4;
        const f32x4 z = (half ? acc1[r] : acc0[r]) + ld4(a.comp_s + (size_t)b * npad + col) + ld4(a.comp_t + (size_t)tk * npad + col);
        if (col + 4 <= a.cut_len) {
          st4(a.za + gr * a.ldza + col, z);
        } else if (col >= a.cut_len && col + 4 <= a.hidden && yvec) {
          f32x4 o;
#pragma unroll
          for (int t = 0; t < 4; ++t) o[t] = relu_nan(z[t]);
          st4(a.y + gr * a.ldy + col, o);
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int c = col + t;
            if (c < cpad) a.za[gr * a.ldza + c] = z[t];     // (pad columns of the aggregation's input rows are read: keep them finite)
            if (c >= a.cut_len && c < a.hidden) a.y[gr * a.ldy + c] = relu_nan(z[t]);
          }
        }
      }
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// partial image of one workgroup: [dC 50 x npad | dT 4 x npad | dW1 25 x 63 | db1 25 | dW2 50 x 25 | db2 50]
constexpr int kW1N = kH1 * kE, kW2N = kH2 * kH1;
__host__ __device__ inline size_t slab_floats(int npad) { return (size_t)(kH2 + 4) * npad + kW1N + kH1 + kW2N + kH2; }
__host__ __device__ inline int c_lds_ld(int npad) { return ((npad / 4) | 1) * 4; }   // an odd number of 16-byte slots per row

template <bool WIDE>
__global__ __launch_bounds__(256) void qnet_bwd_kernel(QnetArgs a, int tiles_per, int wgs_per) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const EncLds L = enc_carve(dyn);
  float *dp2 = dyn + kEncFloats;               // [64][52] gradient before the second ReLU
  float *dp1 = dp2 + kRows * kLdH2;            // [64][28] gradient before the first ReLU
  float *Cl = dp1 + kRows * kLdH1;             // [50][ldcl] the composite C
  const int npad = pad4(a.hidden), nq = npad / 4, ldcl = c_lds_ld(npad);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / wgs_per, g0 = blockIdx.x - b * wgs_per;
  const bool on0 = lane < nq, on1 = WIDE && lane + 64 < nq;
  const float *__restrict__ dz = a.dz;

  enc_load_weights(L, a);
  for (int i = tid; i < kH2 * nq; i += 256) {
    const int k = i / nq, q = i - k * nq;
    st4(Cl + k * ldcl + q * 4, ld4(a.comp_c + (size_t)k * npad + q * 4));
  }

  f32x4 accC0[kKGroup], accC1[kKGroup], accT0 = {0.f, 0.f, 0.f, 0.f}, accT1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < kKGroup; ++i) accC0[i] = accC1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float accW2[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, accW1[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, accB2 = 0.f, accB1 = 0.f;

  for (int t = g0; t < tiles_per; t += wgs_per) {
    const int v0 = t * kRows;
    const int nrows = a.n_vert - v0 < kRows ? a.n_vert - v0 : kRows;
    const size_t gr0 = (size_t)b * a.n_vert + v0;
    __syncthreads();   // the previous tile's readers are done (and, first time round, the weights and C are in LDS after enc_tile's barriers)
    enc_tile(L, a.mesh + (size_t)b * a.n_vert * 4, v0, nrows);

    // dh2[row][k] = sum_j dZ[row][j] C[k][j]: wave = 16 rows, lane = k; the dZ row is the same address for the whole wave
    {
      const int k = lane < kLdH2 ? lane : kLdH2 - 1;
      const float *crow = Cl + (k < kH2 ? k : 0) * ldcl;
      float acc[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int jq = 0; jq < nq; ++jq) {
        const f32x4 cv = ld4(crow + jq * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wave * 16 + r;
          if (row < nrows) {
            const f32x4 d = ld4(dz + (gr0 + row) * npad + jq * 4);
            acc[r] = fmaf(d[0], cv[0], fmaf(d[1], cv[1], fmaf(d[2], cv[2], fmaf(d[3], cv[3], acc[r]))));
          }
        }
      }
      if (lane < kLdH2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wave * 16 + r;
          dp2[row * kLdH2 + k] = (k < kH2 && L.h2[row * kLdH2 + k] > 0.f) ? acc[r] : 0.f;
        }
      }
    }
    __syncthreads();

    // dC[k][cols] += h2[row][k] dZ[row][cols] for this wave's 13 rows of C; token `wave`'s column sums of dZ
    for (int row = 0; row < nrows; ++row) {
      const f32x4 d0 = on0 ? ld4(dz + (gr0 + row) * npad + lane * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 d1 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (on1) d1 = ld4(dz + (gr0 + row) * npad + (lane + 64) * 4);
      const float *hr = L.h2 + row * kLdH2 + wave * kKGroup;
#pragma unroll
      for (int i = 0; i < kKGroup; ++i) {
        const float hk = hr[i];
        accC0[i] += hk * d0;
        if (WIDE) accC1[i] += hk * d1;
      }
      if (L.tok[row] == wave) {
        accT0 += d0;
        if (WIDE) accT1 += d1;
      }
    }
    // dW2[k][i] += dp2[row][k] h1[row][i], db2[k] += dp2[row][k] (rows past nrows hold zeros)
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int o = tid + 256 * s;
      if (o < kW2N) {
        const int k = o / kH1, i = o - k * kH1;
        float acc = 0.f;
        for (int row = 0; row < kRows; ++row) acc = fmaf(dp2[row * kLdH2 + k], L.h1[row * kLdH1 + i], acc);
        accW2[s] += acc;
      }
    }
    if (tid < kH2) {
      float acc = 0.f;
      for (int row = 0; row < kRows; ++row) acc += dp2[row * kLdH2 + tid];
      accB2 += acc;
    }
    // dh1 = dp2 W2, through the first ReLU
    for (int o = tid; o < kRows * kLdH1; o += 256) {
      const int row = o / kLdH1, i = o - row * kLdH1;
      float acc = 0.f;
      if (i < kH1 && L.h1[o] > 0.f) {
#pragma unroll 5
        for (int k = 0; k < kH2; ++k) acc = fmaf(dp2[row * kLdH2 + k], L.w2[k * kH1 + i], acc);
      }
      dp1[o] = acc;
    }
    __syncthreads();
    // dW1[i][c] += dp1[row][i] e[row][c], db1[i] += dp1[row][i]
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const int o = tid + 256 * s;
      if (o < kW1N) {
        const int i = o / kE, c = o - i * kE;
        float acc = 0.f;
        for (int row = 0; row < kRows; ++row) acc = fmaf(dp1[row * kLdH1 + i], L.e[row * kLdE + c], acc);
        accW1[s] += acc;
      }
    }
    if (tid < kH1) {
      float acc = 0.f;
      for (int row = 0; row < kRows; ++row) acc += dp1[row * kLdH1 + tid];
      accB1 += acc;
    }
  }

  float *out = a.slab + (size_t)blockIdx.x * slab_floats(npad);
#pragma unroll
  for (int i = 0; i < kKGroup; ++i) {
    const int k = wave * kKGroup + i;
    if (k < kH2) {
      if (on0) st4(out + (size_t)k * npad + lane * 4, accC0[i]);
      if (on1) st4(out + (size_t)k * npad + (lane + 64) * 4, accC1[i]);
    }
  }
  float *ot = out + (size_t)kH2 * npad + (size_t)wave * npad;
  if (on0) st4(ot + lane * 4, accT0);
  if (on1) st4(ot + (lane + 64) * 4, accT1);
  float *ow = out + (size_t)(kH2 + 4) * npad;
#pragma unroll
  for (int s = 0; s < 7; ++s)
    if (tid + 256 * s < kW1N) ow[tid + 256 * s] = accW1[s];
  if (tid < kH1) ow[kW1N + tid] = accB1;
#pragma unroll
  for (int s = 0; s < 5; ++s)
    if (tid + 256 * s < kW2N) ow[kW1N + kH1 + tid + 256 * s] = accW2[s];
  if (tid < kH2) ow[kW1N + kH1 + kW2N + tid] = accB2;
}

struct QnetOut {
  float *d_s, *d_t, *d_c, *dw1, *db1, *dw2, *db2;
};

// out[i] = sum over the workgroups' images, ascending; dS[b] = the token sums of sample b's workgroups
__global__ void qnet_reduce_kernel(const float *__restrict__ slab, int wgs, int wgs_per, int batch, int npad, QnetOut o) {
  const size_t P = slab_floats(npad);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) {
    float acc = 0.f;
    for (int w = 0; w < wgs; ++w) acc += slab[(size_t)w * P + i];
    const size_t nc = (size_t)kH2 * npad, nt = (size_t)4 * npad;
    size_t j = i;
    float *dst;
    if (j < nc) dst = o.d_c;
    else if ((j -= nc) < nt) dst = o.d_t;
    else if ((j -= nt) < (size_t)kW1N) dst = o.dw1;
    else if ((j -= kW1N) < (size_t)kH1) dst = o.db1;
    else if ((j -= kH1) < (size_t)kW2N) dst = o.dw2;
    else { j -= kW2N; dst = o.db2; }
    dst[j] = acc;
  } else if (i < P + (size_t)batch * npad) {
    const size_t j = i - P;
    const int b = (int)(j / npad), c = (int)(j - (size_t)b * npad);
    float acc = 0.f;
    for (int w = 0; w < wgs_per; ++w)
      for (int t = 0; t < 4; ++t) acc += slab[(size_t)(b * wgs_per + w) * P + (size_t)(kH2 + t) * npad + c];
    o.d_s[j] = acc;
  }
}

int bwd_wgs_per(int batch, int n_vert) {
  const int tiles_per = cdiv(n_vert, kRows);
  int per = kBwdWgs / batch;
  if (per < 1) per = 1;
  return per < tiles_per ? per : tiles_per;
}

}  // namespace

size_t qnet_slab_floats(int hidden) { return slab_floats(pad4(hidden)); }
int qnet_bwd_wgs(int batch, int n_vert) { return batch * bwd_wgs_per(batch, n_vert); }

int launch_qnet_fwd(const QnetArgs &a, hipStream_t s) {
  const int tiles_per = cdiv(a.n_vert, kRows);
  const dim3 grid((unsigned)((long long)a.batch * tiles_per));
  if (pad4(a.hidden) / 4 > 64)
    A3VT_LAUNCH(qnet_fwd_kernel<true>, grid, dim3(256), 0, s, a, tiles_per);
  else
    A3VT_LAUNCH(qnet_fwd_kernel<false>, grid, dim3(256), 0, s, a, tiles_per);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_qnet_bwd(const QnetArgs &a, float *d_s, float *d_t, float *d_c, float *dw1, float *db1, float *dw2, float *db2, hipStream_t s) {
  const int npad = pad4(a.hidden), tiles_per = cdiv(a.n_vert, kRows), per = bwd_wgs_per(a.batch, a.n_vert), wgs = a.batch * per;
  const size_t lds = (size_t)(kEncFloats + kRows * kLdH2 + kRows * kLdH1 + kH2 * c_lds_ld(npad)) * sizeof(float);
  static OncePerDevice once[2];
  const bool wide = npad / 4 > 64;
  hipError_t attr = hipSuccess;
  once[wide].run([&] {
    attr = wide ? hipFuncSetAttribute(reinterpret_cast<const void *>(&qnet_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)
                : hipFuncSetAttribute(reinterpret_cast<const void *>(&qnet_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
  if (attr != hipSuccess) {
    set_error("qnet_input_bwd: cannot raise the dynamic LDS limit: %s", hipGetErrorString(attr));
    return -2;
  }
  if (wide)
    A3VT_LAUNCH(qnet_bwd_kernel<true>, dim3(wgs), dim3(256), lds, s, a, tiles_per, per);
  else
    A3VT_LAUNCH(qnet_bwd_kernel<false>, dim3(wgs), dim3(256), lds, s, a, tiles_per, per);
  A3VT_CHECK_LAUNCH();
  const QnetOut o{d_s, d_t, d_c, dw1, db1, dw2, db2};
  const size_t n = slab_floats(npad) + (size_t)a.batch * npad;
  A3VT_LAUNCH(qnet_reduce_kernel, dim3((unsigned)cdiv((long long)n, 256)), dim3(256), 0, s, a.slab, wgs, per, a.batch, npad, o);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
