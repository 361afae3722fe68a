// conv5f.hip — the fp32 5 x 5 convolutions of the touch chart predictor's stem on channels-last maps: `Encoder` (reference:
// pterotactyl/reconstruction/touch/model.py:10-47) runs nine of them in its first three `DoubleConv` blocks, (cin, cout, stride) =
// (3,16,2), (16,16,1) x 2, (16,32,2), (32,32,1) x 2, (32,32,2), (32,32,1) x 2 on 121^2 ... 16^2 maps with padding 2: 133 M of the
// network's 170 M multiply-adds per image.  This is conv5.hip's recipe on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fmaf chain).
//
// Choices:
//  * Tile: a workgroup of four waves owns 16 output pixels of TH output rows, TH = 16 with 16 output channels and 8 with 32.  Every
//    wave owns FOUR rows and ONE block of 16 output channels (cout = 32: waves 0/1 rows 0-3, waves 2/3 rows 4-7, block = wave & 1),
//    so a wave keeps four independent accumulators (the instruction's 40-cycle dependent latency against its 32-cycle issue) and
//    each weight fragment it holds feeds four MFMAs.
//  * K is NOT split over waves: every output element is one accumulator's chain over the k index in a fixed order — bit-repeatable,
//    and independent of the batch and of the workgroup order by construction.  No atomics.
//  * k index = (tap, input channel).  A lane's B operand for FOUR consecutive MFMAs is ONE 16-byte LDS read: lane (pixel n = lane & 15,
//    q = lane >> 4) reads channels 4 q .. 4 q + 3 of a tap of its pixel, and MFMA j takes element j, i.e. k-slot q of MFMA j is channel
//    4 q + j (32 input channels: two reads per tap, channels 16 h + 4 q + j).  K = 400 -> 100 MFMAs, K = 800 -> 200 per 16 pixels x 16
//    channels.  The 3-channel layer pads a pixel to 4 channels in LDS (the map itself stays 12 bytes per pixel); there k-slot q of
//    step s is TAP 4 s + q and MFMA j channel j < 3: 7 steps x 3 = 21 MFMAs (K = 75 padded to 84; taps 25 .. 27 have zero weights
//    and read a clamped address).
//  * The weight image holds the A fragments in that order, [16-channel block][MFMA index / 4][lane][4] fp32: 16-byte loads, one
//    block per wave, in registers for the whole tile: 100 (cin 16), 200 (cin 32) or 24 (cin 3) registers per lane, next to the four
//    accumulators (16) and the B fragments in flight.  Compiled (gfx950, no scratch): 42 VGPR + 20 AGPR (3,16,2), 147 + 20 (16,16,1),
//    196 + 20 (16,32,2), 255 + 48 (32,32,1), 255 + 128 (32,32,2) — the 32-channel shapes overflow the vector file into accumulation
//    registers (the launch bound of 256 threads allows 512 in all) and run one wave per SIMD.
//  * LDS: the input patch, (TH - 1) stride + 5 rows of 15 stride + 5 pixels: 19.6 KB (3,16,2), 25.6 KB (16,16,1), 42.6 KB (16,32,2),
//    30.7 KB (32,32,1), 85.1 KB (32,32,2).  Pixels outside the map are written as zeros.  Staged through registers (16-byte global
//    loads, 16-byte LDS writes).
//  * Epilogue in registers: D[m = channel][n = pixel] leaves a lane with channels 4 q .. 4 q + 3 of its pixel: scale, shift, ReLU, one
//    16-byte store per row; a wave instruction writes 16 pixels x 64 bytes.
// The K loop is MFMAs and LDS reads only (fp32 MFMA and the vector ALU share a pipe: profiles/r06_fp32_pipe_ubench.txt).
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {


constexpr int kTaps = 25;
constexpr int kTileW = 16;

template <int CIN, int COUT, int STRIDE>
struct C5F {
  static constexpr int kCP = CIN == 3 ? 4 : CIN;                     // channels of a pixel in LDS
  static constexpr int kPix = kCP * 4;                               // bytes of a pixel in LDS
  static constexpr int kTH = COUT == 32 ? 8 : 16;                    // output rows of a tile
  static constexpr int kPW = (kTileW - 1) * STRIDE + 5, kPH = (kTH - 1) * STRIDE + 5;
  static constexpr int kPatchBytes = kPH * kPW * kPix;
  static constexpr int kF4 = CIN == 3 ? 6 : kTaps * CIN / 16;        // groups of four MFMAs (cin 3: 21 used of 24)
};

struct Conv5fArgs {
  const float *x;       // [B][H][W][CIN]
  float *y;             // [B][Ho][Wo][COUT]
  const float *wfrag;   // conv5f_weight_image_kernel
  const float *scale, *shift;   // optional [COUT]
  int B, H, W, Ho, Wo, pad, relu, tiles_x, tiles_y;
};

// A fragments: image[(mb * F4 + g) * 64 + lane][e] = the weight lane (m = lane & 15, q = lane >> 4) feeds to MFMA 4 g + e of channel
// block mb: W[co = 16 mb + m][ci][tap] with, for MFMA index f = 4 g + e,
//   cin 16: tap = f / 4,  ci = 4 q + f % 4;     cin 32: tap = f / 8,  ci = 16 ((f / 4) & 1) + 4 q + f % 4;
//   cin 3:  tap = 4 (f / 3) + q, ci = f % 3  (f < 21; tap >= 25 and f >= 21: zero)
__global__ void conv5f_weight_image_kernel(const float *__restrict__ w, int cout, int cin, float *__restrict__ out) {
  const int f4 = cin == 3 ? 6 : kTaps * cin / 16;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (cout / 16) * f4 * 256) return;
  const int e = i & 3, lane = (i >> 2) & 63, g = (i >> 8) % f4, mb = (i >> 8) / f4;
  const int m = lane & 15, q = lane >> 4, f = 4 * g + e;
  int tap, ci;
  if (cin == 3) {
    tap = f < 21 ? 4 * (f / 3) + q : kTaps;
    ci = f % 3;
  } else if (cin == 16) {
    tap = f >> 2;
    ci = 4 * q + (f & 3);
  } else {
    tap = f >> 3;
    ci = 16 * ((f >> 2) & 1) + 4 * q + (f & 3);
  }
  out[i] = tap < kTaps ? w[((size_t)(mb * 16 + m) * cin + ci) * kTaps + tap] : 0.f;
}

template <int CIN, int COUT, int STRIDE>
__global__ __launch_bounds__(256) void conv5f_kernel(Conv5fArgs a) {
  using S = C5F<CIN, COUT, STRIDE>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), l16 = lane & 15, q = lane >> 4;
  const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y, b = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int ox0 = tx * kTileW, oy0 = ty * S::kTH;
  // ---- the input patch: patch pixel (py, px) is map pixel (oy0 STRIDE + py - pad, ox0 STRIDE + px - pad)
  {
    const float *xb = a.x + (size_t)b * a.H * a.W * CIN;
    if (CIN == 3) {
      for (int p = t; p < S::kPH * S::kPW; p += 256) {
        const int py = p / S::kPW, px = p - py * S::kPW;
        const int iy = oy0 * STRIDE + py - a.pad, ix = ox0 * STRIDE + px - a.pad;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
          const float *src = xb + ((size_t)iy * a.W + ix) * 3;
          v = f32x4{src[0], src[1], src[2], 0.f};
        }
        *reinterpret_cast<f32x4 *>(lds + p * 16) = v;
      }
    } else {
      constexpr int kPP = S::kCP / 4;                             // 16-byte pieces per pixel
      constexpr int kPieces = S::kPH * S::kPW * kPP;
      for (int i = t; i < kPieces; i += 256) {
        const int p = i / kPP, part = i - p * kPP;
        const int py = p / S::kPW, px = p - py * S::kPW;
        const int iy = oy0 * STRIDE + py - a.pad, ix = ox0 * STRIDE + px - a.pad;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
          v = *reinterpret_cast<const f32x4 *>(xb + ((size_t)iy * a.W + ix) * CIN + part * 4);
        *reinterpret_cast<f32x4 *>(lds + i * 16) = v;
      }
    }
  }
  // ---- this wave's rows and channel block; its A fragments
  const int mb = COUT == 32 ? (wave & 1) : 0, r0 = (COUT == 32 ? (wave >> 1) : wave) * 4;
  f32x4 wf[S::kF4];
  {
    const f32x4 *wi = reinterpret_cast<const f32x4 *>(a.wfrag) + (size_t)mb * S::kF4 * 64 + lane;
#pragma unroll
    for (int g = 0; g < S::kF4; ++g) wf[g] = wi[g * 64];
  }
  __syncthreads();
  f32x4 acc[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) acc[rr] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int kRow = STRIDE * S::kPW * S::kPix;                  // bytes between the patch rows of consecutive output rows
  if constexpr (CIN == 3) {
    const char *base = lds + (r0 * STRIDE * S::kPW + l16 * STRIDE) * S::kPix;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      int tap = 4 * s + q;
      tap = tap < kTaps ? tap : kTaps - 1;                         // (taps 25 .. 27: zero weights; any finite pixel will do)
      const int off = ((tap / 5) * S::kPW + tap % 5) * S::kPix;
      f32x4 pix[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) pix[rr] = *reinterpret_cast<const f32x4 *>(base + rr * kRow + off);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int f = 3 * s + j;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[rr] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[f >> 2][f & 3], pix[rr][j], acc[rr], 0, 0, 0);
      }
    }
  } else {
    const char *base = lds + (r0 * STRIDE * S::kPW + l16 * STRIDE) * S::kPix + q * 16;
    constexpr int kH = CIN / 16;
#pragma unroll
    for (int g = 0; g < S::kF4; ++g) {
      const int tap = g / kH, h = g % kH;
      const int off = ((tap / 5) * S::kPW + tap % 5) * S::kPix + h * 64;
      f32x4 pix[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) pix[rr] = *reinterpret_cast<const f32x4 *>(base + rr * kRow + off);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[rr] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[g][j], pix[rr][j], acc[rr], 0, 0, 0);
    }
  }
  // ---- epilogue: this lane holds channels c0 .. c0 + 3 of pixel l16 of its four rows
  const int c0 = mb * 16 + 4 * q;
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (a.scale) sc = f32x4{a.scale[c0], a.scale[c0 + 1], a.scale[c0 + 2], a.scale[c0 + 3]};
  if (a.shift) sh = f32x4{a.shift[c0], a.shift[c0 + 1], a.shift[c0 + 2], a.shift[c0 + 3]};
  const int ox = ox0 + l16;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int oy = oy0 + r0 + rr;
    if (oy < a.Ho && ox < a.Wo) {
      f32x4 v = acc[rr] * sc + sh;
      if (a.relu) v = f32x4{relu_nan(v[0]), relu_nan(v[1]), relu_nan(v[2]), relu_nan(v[3])};
      *reinterpret_cast<f32x4 *>(a.y + (((size_t)b * a.Ho + oy) * a.Wo + ox) * COUT + c0) = v;
    }
  }
}

template <int CIN, int COUT, int STRIDE>
int conv5f_launch(Conv5fArgs a, hipStream_t s) {
  using S = C5F<CIN, COUT, STRIDE>;
  static OncePerDevice once;
  hipError_t attr = hipSuccess;
  once.run([&attr] {
    attr = hipFuncSetAttribute((const void *)conv5f_kernel<CIN, COUT, STRIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, S::kPatchBytes);
  });
  if (attr != hipSuccess) {     // (32,32,2) needs 85 KB of dynamic LDS, above the 64 KB a kernel gets without the attribute
    set_error("conv5f: cannot raise the dynamic LDS limit of the %d -> %d stride %d kernel to %d bytes: %s", CIN, COUT, STRIDE, S::kPatchBytes,
              hipGetErrorString(attr));
    return -2;
  }
  a.tiles_x = (a.Wo + kTileW - 1) / kTileW;
  a.tiles_y = (a.Ho + S::kTH - 1) / S::kTH;
  A3VT_LAUNCH((conv5f_kernel<CIN, COUT, STRIDE>), dim3((unsigned)(a.B * a.tiles_x * a.tiles_y)), dim3(256), S::kPatchBytes, s, a);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace

bool conv5f_shape_ok(int cin, int cout, int stride) {
  return (cin == 3 && cout == 16 && stride == 2) || (cin == 16 && cout == 16 && stride == 1) || (cin == 16 && cout == 32 && stride == 2) ||
         (cin == 32 && cout == 32 && stride == 1) || (cin == 32 && cout == 32 && stride == 2);
}

size_t conv5f_weight_image_bytes(int cin, int cout) {
  const bool ok = (cin == 3 && cout == 16) || (cin == 16 && (cout == 16 || cout == 32)) || (cin == 32 && cout == 32);
  return ok ? (size_t)(cout / 16) * (cin == 3 ? 6 : kTaps * cin / 16) * 256 * sizeof(float) : 0;
}

int launch_conv5f_weight_image(const float *w, int cout, int cin, void *image, hipStream_t s) {
  const int n = (int)(conv5f_weight_image_bytes(cin, cout) / sizeof(float));
  A3VT_LAUNCH(conv5f_weight_image_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w, cout, cin, static_cast<float *>(image));
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_conv5f(const float *x, int batch, int h, int w, int cin, int cout, int stride, int pad, const void *image, const float *scale,
                  const float *shift, int relu, float *y, hipStream_t s) {
  Conv5fArgs a{};
  a.x = x;
  a.y = y;
  a.wfrag = static_cast<const float *>(image);
  a.scale = scale;
  a.shift = shift;
  a.B = batch;
  a.H = h;
  a.W = w;
  a.pad = pad;
  a.relu = relu;
  a.Ho = (h + 2 * pad - 5) / stride + 1;
  a.Wo = (w + 2 * pad - 5) / stride + 1;
  if (cin == 3 && cout == 16 && stride == 2) return conv5f_launch<3, 16, 2>(a, s);
  if (cin == 16 && cout == 16 && stride == 1) return conv5f_launch<16, 16, 1>(a, s);
  if (cin == 16 && cout == 32 && stride == 2) return conv5f_launch<16, 32, 2>(a, s);
  if (cin == 32 && cout == 32 && stride == 1) return conv5f_launch<32, 32, 1>(a, s);
  if (cin == 32 && cout == 32 && stride == 2) return conv5f_launch<32, 32, 2>(a, s);
  set_error("conv5f: shape %d -> %d stride %d not taken", cin, cout, stride);
  return -1;
}

}  // namespace a3vt
