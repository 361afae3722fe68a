// touch_render.hip — the rendered half of the reference's touch simulator: from a finger frame and the object's triangles to the
// depth map, the contact status, the RGB gel image and the contact point cloud of every finger view of a batch.
//
// Reference: pterotactyl/simulator/scene/instance.py:121-151 (a 121 x 121 pyrender depth camera at the finger, the status),
// :207-258 (depth_to_touch) and :154-204 (depth_to_points), one finger at a time on the host.  Here: TWO launches for the batch.
//
//   touch_depth   one workgroup of 256 threads per 16 x 16 pixel tile of one image.  The mesh's faces are taken 256 at a time:
//                 thread t tests face t's bounding sphere, moved to the camera frame, against the four side planes of the tile's
//                 pyramid and the depth range; the survivors are ballot-compacted into LDS as 13 floats each; then every thread
//                 casts its pixel's ray at the survivors.  min() is exact, so neither the chunking nor the survivors' order shows.
//                 The hit test is watertight: a face's three edge functions are d . (a x b) with the cross product of an edge
//                 always formed from the vertex of the lower index to the higher (negated for the other winding) in explicitly
//                 rounded steps, so the two faces of a shared edge see the same number with opposite signs and a ray cannot pass
//                 between them; the test is inclusive (all three >= 0 or all three <= 0: two-sided).  The depth is
//                 (v0 . n) / (d . n) with n from the face's edges — d = (x, y, -1) in the eye frame, so it is -z of the hit.
//   touch_finish  one workgroup of 1024 threads per image, thread t owning the 15 consecutive pixels from 15 t (row-major), the gel
//                 map in LDS.  Status and kept-point counts are integer sums; the 7 x 7 means are taken into registers before any
//                 of them is written back; the points are compacted in pixel order by a prefix sum over the threads.
// No atomics, no workspace, every float sum in a fixed order: the same bits on every call, whatever else is in the batch.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace a3vt {

namespace {

constexpr int kRes = kTouchRes, kPix = kTouchRes * kTouchRes;
constexpr int kTile = 16, kTilesAcross = (kRes + kTile - 1) / kTile, kTilesPerImage = kTilesAcross * kTilesAcross;
constexpr int kDepthThreads = kTile * kTile;
static_assert(kDepthThreads == kTouchFaceChunk, "a thread tests one face of a chunk");
constexpr int kRecord = 13;   // c0, c1, c2 (the edge functions' vectors), n, v0 . n
constexpr int kFinishThreads = 1024, kPerThread = 15;
static_assert(kFinishThreads * kPerThread >= kPix, "every pixel has a thread");

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// Explicitly rounded (no contraction the compiler may choose differently from one call site to the next): what makes the edge
// functions of a shared edge equal in magnitude in both faces.
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {__fmaf_rn(a.y, b.z, -__fmul_rn(a.z, b.y)), __fmaf_rn(a.z, b.x, -__fmul_rn(a.x, b.z)),
          __fmaf_rn(a.x, b.y, -__fmul_rn(a.y, b.x))};
}
__device__ __forceinline__ float dot(V3 a, V3 b) { return __fmaf_rn(a.x, b.x, __fmaf_rn(a.y, b.y, __fmul_rn(a.z, b.z))); }
__device__ __forceinline__ V3 edge_vector(V3 a, V3 b, int ia, int ib) {   // a x b, formed lower index first
  if (ia <= ib) return cross(a, b);
  const V3 c = cross(b, a);
  return {-c.x, -c.y, -c.z};
}

// The camera rotation C = R . R_y(-90 deg) (instance.py:127-133): its columns are (R[:, 2], R[:, 1], -R[:, 0]); row-major.
struct Camera {
  float c[9], p[3];
};
__device__ __forceinline__ Camera load_camera(const float *cam_pos, const float *cam_rot, long long img) {
  Camera cam;
  const float *R = cam_rot + 9 * img;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    cam.c[3 * i + 0] = R[3 * i + 2];
    cam.c[3 * i + 1] = R[3 * i + 1];
    cam.c[3 * i + 2] = -R[3 * i + 0];
    cam.p[i] = cam_pos[3 * img + i];
  }
  return cam;
}
__device__ __forceinline__ V3 to_eye(const Camera &cam, V3 w) {   // C^T (w - p)
  const V3 d = {w.x - cam.p[0], w.y - cam.p[1], w.z - cam.p[2]};
  return {dot({cam.c[0], cam.c[3], cam.c[6]}, d), dot({cam.c[1], cam.c[4], cam.c[7]}, d), dot({cam.c[2], cam.c[5], cam.c[8]}, d)};
}

__global__ __launch_bounds__(kDepthThreads) void touch_depth_kernel(const float *__restrict__ verts, int V,
                                                                    const int32_t *__restrict__ faces, int F,
                                                                    const int32_t *__restrict__ face_offset, int M,
                                                                    const int32_t *__restrict__ image_mesh,
                                                                    const float *__restrict__ cam_pos, const float *__restrict__ cam_rot,
                                                                    float tan_half, float znear, float zfar, float *__restrict__ depth) {
  __shared__ float rec_s[kRecord][kTouchFaceChunk];
  __shared__ int wave_n[kDepthThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long img = blockIdx.x / kTilesPerImage;
  const int tile = blockIdx.x % kTilesPerImage, ty = tile / kTilesAcross, tx = tile % kTilesAcross;
  const int r = ty * kTile + tid / kTile, c = tx * kTile + tid % kTile;

  const int m = min(max(image_mesh[img], 0), M - 1);
  const int f0 = min(max(face_offset[m], 0), F), f1 = min(max(face_offset[m + 1], f0), F);
  const Camera cam = load_camera(cam_pos, cam_rot, img);

  // the pixel's ray and the tile's pyramid (pixel edges; the last tiles end with the image)
  const V3 d = {((c + 0.5f) / kRes * 2.f - 1.f) * tan_half, (1.f - (r + 0.5f) / kRes * 2.f) * tan_half, -1.f};
  const float xl = ((float)(tx * kTile) / kRes * 2.f - 1.f) * tan_half;
  const float xr = ((float)min(tx * kTile + kTile, kRes) / kRes * 2.f - 1.f) * tan_half;
  const float yt = (1.f - (float)(ty * kTile) / kRes * 2.f) * tan_half;
  const float yb = (1.f - (float)min(ty * kTile + kTile, kRes) / kRes * 2.f) * tan_half;
  const float il = rsqrtf(1.f + xl * xl), ir = rsqrtf(1.f + xr * xr), it = rsqrtf(1.f + yt * yt), ib = rsqrtf(1.f + yb * yb);

  float best = INFINITY;
  for (int base = f0; base < f1; base += kTouchFaceChunk) {
    const int f = base + tid;
    bool keep = false;
    int i0 = 0, i1 = 0, i2 = 0;
    V3 a = {}, b = {}, e = {};
    if (f < f1) {
      i0 = faces[3ll * f], i1 = faces[3ll * f + 1], i2 = faces[3ll * f + 2];
      if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {   // (others are skipped)
        a = {verts[3ll * i0], verts[3ll * i0 + 1], verts[3ll * i0 + 2]};
        b = {verts[3ll * i1], verts[3ll * i1 + 1], verts[3ll * i1 + 2]};
        e = {verts[3ll * i2], verts[3ll * i2 + 1], verts[3ll * i2 + 2]};
        const V3 g = {(a.x + b.x + e.x) * (1.f / 3.f), (a.y + b.y + e.y) * (1.f / 3.f), (a.z + b.z + e.z) * (1.f / 3.f)};
        const V3 da = sub(a, g), db = sub(b, g), de = sub(e, g);
        const float rad = sqrtf(fmaxf(dot(da, da), fmaxf(dot(db, db), dot(de, de))));
        const V3 q = to_eye(cam, g);
        const float w = -q.z;
        // generous against the rounding of the centre and the radius: the cull may keep too much, never too little
        const float rs = rad * 1.001f + 1e-6f * (fabsf(q.x) + fabsf(q.y) + fabsf(w));
        keep = (q.x - xl * w) * il >= -rs && (xr * w - q.x) * ir >= -rs && (q.y - yb * w) * ib >= -rs && (yt * w - q.y) * it >= -rs &&
               w + rs >= znear && w - rs <= zfar;
      }
    }
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(vote);
    __syncthreads();
    int slot = __popcll(vote & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < kDepthThreads / kWave; ++w) {
      if (w < wave) slot += wave_n[w];
      total += wave_n[w];
    }
    if (keep) {
      const V3 v0 = to_eye(cam, a), v1 = to_eye(cam, b), v2 = to_eye(cam, e);
      const V3 c0 = edge_vector(v1, v2, i1, i2), c1 = edge_vector(v2, v0, i2, i0), c2 = edge_vector(v0, v1, i0, i1);
      const V3 n = cross(sub(v1, v0), sub(v2, v0));
      rec_s[0][slot] = c0.x, rec_s[1][slot] = c0.y, rec_s[2][slot] = c0.z;
      rec_s[3][slot] = c1.x, rec_s[4][slot] = c1.y, rec_s[5][slot] = c1.z;
      rec_s[6][slot] = c2.x, rec_s[7][slot] = c2.y, rec_s[8][slot] = c2.z;
      rec_s[9][slot] = n.x, rec_s[10][slot] = n.y, rec_s[11][slot] = n.z;
      rec_s[12][slot] = dot(v0, n);
    }
    __syncthreads();
    for (int j = 0; j < total; ++j) {   // (every lane reads the same LDS word: a broadcast)
      const float u0 = dot(d, {rec_s[0][j], rec_s[1][j], rec_s[2][j]});
      const float u1 = dot(d, {rec_s[3][j], rec_s[4][j], rec_s[5][j]});
      const float u2 = dot(d, {rec_s[6][j], rec_s[7][j], rec_s[8][j]});
      if ((u0 >= 0.f && u1 >= 0.f && u2 >= 0.f) || (u0 <= 0.f && u1 <= 0.f && u2 <= 0.f)) {
        const float t = __fdiv_rn(rec_s[12][j], dot(d, {rec_s[9][j], rec_s[10][j], rec_s[11][j]}));
        if (t >= znear && t <= zfar) best = fminf(best, t);   // (a NaN, from a face seen edge-on, fails both)
      }
    }
    __syncthreads();   // (the records are read; the next chunk may overwrite them)
  }
  if (r < kRes && c < kRes) depth[img * kPix + r * kRes + c] = best == INFINITY ? 0.f : best;
}

__device__ __forceinline__ int reflect(int i) { return i < 0 ? -1 - i : (i >= kRes ? 2 * kRes - 1 - i : i); }   // d c b a | a b c d

__global__ __launch_bounds__(kFinishThreads) void touch_finish_kernel(const float *__restrict__ depth, const float *__restrict__ cam_pos,
                                                                      const float *__restrict__ cam_rot, float max_depth, float tan_half,
                                                                      float *__restrict__ touch, float *__restrict__ points,
                                                                      int32_t *__restrict__ count, int32_t *__restrict__ status) {
  __shared__ float gel[kPix];
  __shared__ int wave_keep[kFinishThreads / kWave], wave_contact[kFinishThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long img = blockIdx.x;
  const int p0 = tid * kPerThread;

  // range handling (instance.py:209-220 and :162-166), the status count (:142), the points to keep (:187)
  float dd[kPerThread], mean[kPerThread];
  unsigned zeroed = 0, kept = 0;
  int contact = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int p = p0 + k;
    dd[k] = 1.f, mean[k] = 0.f;
    if (p < kPix) {
      const float v = depth[img * kPix + p];
      contact += (v <= max_depth ? 1 : 0) - (v == 0.f ? 1 : 0);
      dd[k] = (v > max_depth || v == 0.f) ? 1.f : v;
      const bool z = dd[k] >= max_depth;
      float g = z ? 0.f : -(dd[k] - max_depth);
      g = g * 6.f / max_depth;
      gel[p] = g / 30.f + 0.4f;
      zeroed |= (z ? 1u : 0u) << k;
      kept |= (dd[k] < 1.f ? 1u : 0u) << k;
    }
  }
  const int n_keep = __popc(kept);
  int scan = n_keep, csum = contact;   // inclusive scan of the kept counts over the wave; the contacts' sum
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int up = __shfl_up(scan, off, kWave);
    if (lane >= off) scan += up;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) csum += __shfl_xor(csum, off, kWave);
  if (lane == kWave - 1) wave_keep[wave] = scan;
  if (lane == 0) wave_contact[wave] = csum;
  __syncthreads();   // (the gel map is complete too)
  int first = scan - n_keep, total = 0, contacts = 0;
#pragma unroll
  for (int w = 0; w < kFinishThreads / kWave; ++w) {
    if (w < wave) first += wave_keep[w];
    total += wave_keep[w];
    contacts += wave_contact[w];
  }
  if (tid == 0) {
    status[img] = contacts > 0 ? 1 : 0;
    if (count) count[img] = total;
  }

  if (touch) {   // (uniform)
    // 7 x 7 mean, SciPy's "reflect", of the map BEFORE any write-back (:221-226): into registers, then a barrier, then written
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      if (!((zeroed >> k) & 1u)) continue;
      const int p = p0 + k, r = p / kRes, c = p - r * kRes;
      float sum = 0.f;
      for (int dr = -3; dr <= 3; ++dr) {
        const float *row = gel + reflect(r + dr) * kRes;
#pragma unroll
        for (int dc = -3; dc <= 3; ++dc) sum += row[reflect(c + dc)];
      }
      mean[k] = sum * (1.f / 49.f);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k)
      if ((zeroed >> k) & 1u) gel[p0 + k] = mean[k];
    __syncthreads();

    // np.gradient, the normal, three diffuse lights (:229-257)
    const float light[3][3] = {{-0.5f, 0.5f, 1.f}, {1.3f, -0.4f, 1.f}, {1.3f, 1.4f, 1.f}};
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int p = p0 + k;
      if (p >= kPix) break;
      const int r = p / kRes, c = p - r * kRes;
      const float g = gel[p];
      const float zy = r == 0 ? gel[p + kRes] - g : (r == kRes - 1 ? g - gel[p - kRes] : (gel[p + kRes] - gel[p - kRes]) * 0.5f);
      const float zx = c == 0 ? gel[p + 1] - g : (c == kRes - 1 ? g - gel[p - 1] : (gel[p + 1] - gel[p - 1]) * 0.5f);
      const float nn = sqrtf(zx * zx + zy * zy + 1.f);
      const float nx = -zx / nn, ny = -zy / nn, nz = 1.f / nn;
      const float px = (float)r / kRes, py = (float)c / kRes;
      float *out = touch + (img * kPix + p) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float lx = light[ch][0] - px, ly = light[ch][1] - py, lz = light[ch][2] - g;
        const float ln = sqrtf(lx * lx + ly * ly + lz * lz);
        const float v = 2.f * (nx * (lx / ln) + ny * (ly / ln) + nz * (lz / ln));
        out[ch] = fminf(fmaxf(fminf(fmaxf(v, 0.f), 1.f) * 255.f, 0.f), 255.f);
      }
    }
  }

  if (points) {   // (uniform) the reference's grid (:172-184), rotated by the camera rotation and moved to the finger (:191-200)
    const Camera cam = load_camera(cam_pos, cam_rot, img);
    float *out = points + (img * kPix + first) * 3;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      if (!((kept >> k) & 1u)) continue;
      const int p = p0 + k, r = p / kRes, c = p - r * kRes;
      const int xs = c - kRes / 2, ys = r - kRes / 2;
      const float ax = fabsf((float)xs) / (float)(kRes / 2) * tan_half, ay = fabsf((float)ys) / (float)(kRes / 2) * tan_half;
      const float x = dd[k] * ax * (xs > 0 ? 1.f : (xs < 0 ? -1.f : 0.f)), y = dd[k] * ay * (ys > 0 ? -1.f : (ys < 0 ? 1.f : 0.f));
      const float z = -dd[k];
      out[0] = cam.c[0] * x + cam.c[1] * y + cam.c[2] * z + cam.p[0];
      out[1] = cam.c[3] * x + cam.c[4] * y + cam.c[5] * z + cam.p[1];
      out[2] = cam.c[6] * x + cam.c[7] * y + cam.c[8] * z + cam.p[2];
      out += 3;
    }
  }
}

}  // namespace

int launch_touch_depth(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_offset, int M, const int32_t *image_mesh,
                       const float *cam_pos, const float *cam_rot, int I, float yfov, float znear, float zfar, float *depth,
                       hipStream_t s) {
  const float tan_half = (float)tan(0.5 * (double)yfov);
  A3VT_LAUNCH(touch_depth_kernel, dim3((unsigned)I * kTilesPerImage), dim3(kDepthThreads), 0, s, verts, V, faces, F, face_offset, M,
              image_mesh, cam_pos, cam_rot, tan_half, znear, zfar, depth);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_touch_finish(const float *depth, const float *cam_pos, const float *cam_rot, int I, float max_depth, float yfov, float *touch,
                        float *points, int32_t *count, int32_t *status, hipStream_t s) {
  const float tan_half = (float)tan(0.5 * (double)yfov);
  A3VT_LAUNCH(touch_finish_kernel, dim3((unsigned)I), dim3(kFinishThreads), 0, s, depth, cam_pos, cam_rot, max_depth, tan_half, touch,
              points, count, status);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
