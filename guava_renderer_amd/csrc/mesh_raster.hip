// mesh_raster.hip -- mesh visibility rasterizer (include/gsr_mesh.h): PyTorch3D's rasterize_meshes at
// blur_radius = 0, faces_per_pixel = 1, perspective-correct, restated in this project's camera
// convention (the reference's BaseMeshRenderer.render_fragments, utils/graphics_utils.py:471-492),
// for gfx950.
//
// Four launches per call (and the texel gather) on the caller's stream, no host synchronisation:
//   k_mesh_project     one lane per (frame, vertex): (px, py, zv) as one float4.  The same grid also
//                      resets the call's state: the key plane to all-ones, face_visible to 0, the
//                      counters and the worklist length to 0.
//   k_mesh_faces       one lane per (frame, face): culls and bounding box (face_setup).  A face whose
//                      clipped box holds at most kLaneBox pixel centres (SMPL-X at 512^2: ~3) is
//                      rasterized by its lane; a larger one is appended to the worklist [B*F].
//   k_mesh_faces_wide  one wave per worklist face, walking the box 64 pixels at a time.
//   k_mesh_resolve     one lane per pixel: decodes the key, recomputes the barycentrics with the very
//                      function the raster pass used (pixel_eval) and writes the images.
//   k_mesh_texels      (gsr_mesh_visible_texels) face_visible gathered through binding_face.
// Depth test: one 64-bit atomicMin per covered (pixel, face) on  (bits(pz) << 32) | face.  pz >= 0,
// so the bit order is the numeric order, and the face index in the low word breaks ties towards the
// lowest index: the winner is independent of arrival order.
#include "../../include/gsr.h"
#include "../../include/gsr_mesh.h"
#include "gsr_internal.h"

namespace gsr {

constexpr int kLaneBox = 16;         // candidate pixels a face's own lane rasterizes
constexpr int kWideBlocks = 1024;    // k_mesh_faces_wide grid cap (4 waves per block, grid-stride)
constexpr unsigned long long kEmptyKey = ~0ull;

// workspace head: word 0 the worklist length; then kStatSlots 64-byte lines, each holding one share of
// stats[0..3] (lane faces, wide faces, culled faces, covered pixels).  A workgroup adds to line
// blockIdx & (kStatSlots - 1): atomics on one word saturate near 90 per microsecond on this chip, which
// a counter per launch would make the whole call's bound.  gsr_mesh_raster_stats sums the shares.
constexpr int kStatSlots = 64;
constexpr int kHeadWords = 16 + 16 * kStatSlots;
constexpr size_t kHeadBytes = 4 * (size_t)kHeadWords;

__device__ __forceinline__ uint32_t* stat_line(uint32_t* head) {
    return head + 16 + 16 * (blockIdx.x & (kStatSlots - 1));
}

struct MeshLayout {
    uint32_t* head;
    unsigned long long* keys;  // [B*H*W]
    float4* pv;                // [B*V]  (px, py, zv, 0)
    uint32_t* worklist;        // [B*F]  b*F + f
    size_t bytes;
};

static inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

static MeshLayout mesh_layout(void* ws, int B, int V, int F, int W, int H) {
    MeshLayout l;
    char* p = (char*)ws;
    size_t o = 0;
    l.head = (uint32_t*)(p + o);
    o += kHeadBytes;
    l.keys = (unsigned long long*)(p + o);
    o += up256((size_t)B * H * W * 8);
    l.pv = (float4*)(p + o);
    o += up256((size_t)B * V * 16);
    l.worklist = (uint32_t*)(p + o);
    o += up256((size_t)B * F * 4);
    l.bytes = o;
    return l;
}

static bool mesh_sizes_ok(int B, int V, int F, int W, int H) {
    if (B <= 0 || V <= 0 || F <= 0 || W <= 0 || H <= 0 || W > 16384 || H > 16384) return false;
    const int64_t lim = (int64_t)1 << 31;
    return (int64_t)B * V < lim && (int64_t)B * F < lim && (int64_t)B * H * W < lim;
}

struct FaceSetup {
    float x0, y0, z0, x1, y1, z1, x2, y2, z2, area;
    int xlo, xhi, ylo, yhi;  // clipped candidate box (empty when xlo > xhi or ylo > yhi)
    bool ok;                 // passed the culls
};

__device__ __forceinline__ bool finite3(const float4& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

__device__ __forceinline__ FaceSetup face_setup(const float4* __restrict__ pv, const int32_t* __restrict__ faces,
                                                int f, int V, int W, int H) {
    FaceSetup s;
    s.ok = false;
    const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return s;
    const float4 a = pv[i0], b = pv[i1], c = pv[i2];
    s.x0 = a.x, s.y0 = a.y, s.z0 = a.z;
    s.x1 = b.x, s.y1 = b.y, s.z1 = b.z;
    s.x2 = c.x, s.y2 = c.y, s.z2 = c.z;
    if (!(finite3(a) && finite3(b) && finite3(c))) return s;
    if (fmaxf(fmaxf(s.z0, s.z1), s.z2) < 0.f) return s;
    s.area = (s.x2 - s.x0) * (s.y1 - s.y0) - (s.y2 - s.y0) * (s.x1 - s.x0);
    const float thr = 1e-8f * (((float)W * (float)H) * 0.25f);
    if (fabsf(s.area) <= thr) return s;
    const float xmin = fminf(fminf(s.x0, s.x1), s.x2), xmax = fmaxf(fmaxf(s.x0, s.x1), s.x2);
    const float ymin = fminf(fminf(s.y0, s.y1), s.y2), ymax = fmaxf(fmaxf(s.y0, s.y1), s.y2);
    // clamp in float first: the coordinates are finite but may be far outside int's range
    s.xlo = (int)fminf(fmaxf(ceilf(xmin), 0.f), (float)W);
    s.xhi = (int)fminf(fmaxf(floorf(xmax), -1.f), (float)(W - 1));
    s.ylo = (int)fminf(fmaxf(ceilf(ymin), 0.f), (float)H);
    s.yhi = (int)fminf(fmaxf(floorf(ymax), -1.f), (float)(H - 1));
    s.ok = true;
    return s;
}

__device__ __forceinline__ float edge_fn(float px, float py, float ax, float ay, float bx, float by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// the per-pixel test of include/gsr_mesh.h: true when the pixel centre is strictly inside and pz >= 0
__device__ __forceinline__ bool pixel_eval(const FaceSetup& s, int xi, int yi, float& b0, float& b1, float& b2,
                                           float& pz) {
    const float px = (float)xi, py = (float)yi;
    const float w0 = edge_fn(px, py, s.x1, s.y1, s.x2, s.y2) / s.area;
    const float w1 = edge_fn(px, py, s.x2, s.y2, s.x0, s.y0) / s.area;
    const float w2 = edge_fn(px, py, s.x0, s.y0, s.x1, s.y1) / s.area;
    const float t0 = (w0 * s.z1) * s.z2;
    const float t1 = (s.z0 * w1) * s.z2;
    const float t2 = (s.z0 * s.z1) * w2;
    const float d = fmaxf((t0 + t1) + t2, 1e-8f);
    b0 = t0 / d;
    b1 = t1 / d;
    b2 = t2 / d;
    const float z = (b0 * s.z0 + b1 * s.z1) + b2 * s.z2;
    pz = fabsf(z);  // (kept only when z >= 0; fabsf turns -0 into +0, so the bits order like the value)
    return w0 > 0.f && w1 > 0.f && w2 > 0.f && z >= 0.f;
}

__device__ __forceinline__ void depth_test(unsigned long long* __restrict__ keys, int64_t pix, float pz, int f) {
    atomicMin(&keys[pix], ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned)f);
}

// adds the number of active lanes with `flag` to *counter, one atomic per wave
__device__ __forceinline__ void wave_count(uint32_t* counter, bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m != 0 && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(counter, (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(256) k_mesh_project(int B, int V, int F, int W, int H,
                                                      const float* __restrict__ verts,
                                                      const float* __restrict__ w2c,
                                                      const float* __restrict__ tanfovx,
                                                      const float* __restrict__ tanfovy, float4* __restrict__ pv,
                                                      unsigned long long* __restrict__ keys,
                                                      uint8_t* __restrict__ face_visible,
                                                      uint32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < kHeadWords) head[i] = 0;
    if (i < (int64_t)B * H * W) keys[i] = kEmptyKey;
    if (face_visible && i < (int64_t)B * F) face_visible[i] = 0;
    if (i >= (int64_t)B * V) return;
    const int b = (int)(i / V);
    const float* M = w2c + 16 * (int64_t)b;
    const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
    const float xv = (M[0] * x + M[1] * y) + (M[2] * z + M[3]);
    const float yv = (M[4] * x + M[5] * y) + (M[6] * z + M[7]);
    const float zv = (M[8] * x + M[9] * y) + (M[10] * z + M[11]);
    const float den = zv + 1e-7f;
    const float xn = xv / (den * tanfovx[b]);
    const float yn = yv / (den * tanfovy[b]);
    const float px = ((xn + 1.0f) * (float)W - 1.0f) * 0.5f;
    const float py = ((yn + 1.0f) * (float)H - 1.0f) * 0.5f;
    pv[i] = make_float4(px, py, zv, 0.f);
}

__global__ void __launch_bounds__(256) k_mesh_faces(int B, int V, int F, int W, int H,
                                                    const int32_t* __restrict__ faces,
                                                    const float4* __restrict__ pv,
                                                    unsigned long long* __restrict__ keys,
                                                    uint32_t* __restrict__ worklist, uint32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < (int64_t)B * F;
    const int b = live ? (int)(i / F) : 0;
    const int f = live ? (int)(i - (int64_t)b * F) : 0;
    FaceSetup s;
    s.ok = false;
    if (live) s = face_setup(pv + (int64_t)b * V, faces, f, V, W, H);
    const int nx = s.ok ? max(s.xhi - s.xlo + 1, 0) : 0, ny = s.ok ? max(s.yhi - s.ylo + 1, 0) : 0;
    const int64_t n = (int64_t)nx * ny;
    const bool wide = live && s.ok && n > kLaneBox;
    // one atomic per workgroup and counter: the waves' ballots meet in LDS
    __shared__ uint32_t cnt[4][3];
    __shared__ uint32_t wl_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m_wide = __ballot(wide);
    const unsigned long long m_lane = __ballot(live && s.ok && !wide), m_cull = __ballot(live && !s.ok);
    if (lane == 0) {
        cnt[wave][0] = (uint32_t)__popcll(m_lane);
        cnt[wave][1] = (uint32_t)__popcll(m_wide);
        cnt[wave][2] = (uint32_t)__popcll(m_cull);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t t = cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
        if (t) atomicAdd(stat_line(head) + threadIdx.x, t);
        if (threadIdx.x == 1) wl_base = t ? atomicAdd(head, t) : 0u;  // (at most B*F appends in all)
    }
    __syncthreads();
    if (wide) {
        uint32_t at = wl_base + (uint32_t)__popcll(m_wide & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) at += cnt[w][1];
        worklist[at] = (uint32_t)i;
        return;
    }
    if (!live || !s.ok) return;
    unsigned long long* kb = keys + (int64_t)b * H * W;
    for (int yi = s.ylo; yi <= s.yhi; ++yi)
        for (int xi = s.xlo; xi <= s.xhi; ++xi) {
            float b0, b1, b2, pz;
            if (pixel_eval(s, xi, yi, b0, b1, b2, pz)) depth_test(kb, (int64_t)yi * W + xi, pz, f);
        }
}

__global__ void __launch_bounds__(256) k_mesh_faces_wide(int B, int V, int F, int W, int H,
                                                         const int32_t* __restrict__ faces,
                                                         const float4* __restrict__ pv,
                                                         unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ worklist,
                                                         const uint32_t* __restrict__ head) {
    const uint32_t count = min(head[0], (uint32_t)((int64_t)B * F));
    const int lane = threadIdx.x & 63;
    const uint32_t nwaves = gridDim.x * 4u;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < count; w += nwaves) {
        const uint32_t i = worklist[w];
        const int b = (int)(i / (uint32_t)F), f = (int)(i - (uint32_t)b * (uint32_t)F);
        if (b >= B) continue;
        const FaceSetup s = face_setup(pv + (int64_t)b * V, faces, f, V, W, H);
        if (!s.ok) continue;
        const int nx = s.xhi - s.xlo + 1, ny = s.yhi - s.ylo + 1;
        if (nx <= 0 || ny <= 0) continue;
        const int n = nx * ny;  // <= W*H < 2^31
        unsigned long long* kb = keys + (int64_t)b * H * W;
        for (int k = lane; k < n; k += 64) {
            const int ry = k / nx, rx = k - ry * nx;
            const int xi = s.xlo + rx, yi = s.ylo + ry;
            float b0, b1, b2, pz;
            if (pixel_eval(s, xi, yi, b0, b1, b2, pz)) depth_test(kb, (int64_t)yi * W + xi, pz, f);
        }
    }
}

__global__ void __launch_bounds__(256) k_mesh_resolve(int B, int V, int F, int W, int H, int packed,
                                                      const int32_t* __restrict__ faces,
                                                      const float4* __restrict__ pv,
                                                      const unsigned long long* __restrict__ keys,
                                                      int32_t* __restrict__ pix_to_face, float* __restrict__ zbuf,
                                                      float* __restrict__ bary, uint8_t* __restrict__ face_visible,
                                                      uint32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < (int64_t)B * H * W;
    const unsigned long long key = live ? keys[i] : kEmptyKey;
    const bool hit = key != kEmptyKey && (uint32_t)key < (uint32_t)F;
    wave_count(stat_line(head) + 3, hit);
    if (!live) return;
    int32_t face = -1;
    float z = -1.f, b0 = -1.f, b1 = -1.f, b2 = -1.f;
    if (hit) {
        const int b = (int)(i / ((int64_t)H * W));
        const int r = (int)(i - (int64_t)b * H * W);
        const int yi = r / W, xi = r - yi * W;
        const int f = (int)(uint32_t)key;
        const FaceSetup s = face_setup(pv + (int64_t)b * V, faces, f, V, W, H);
        float pz;
        pixel_eval(s, xi, yi, b0, b1, b2, pz);
        z = __uint_as_float((uint32_t)(key >> 32));  // (== pz: the same function on the same operands)
        face = packed ? b * F + f : f;
        if (face_visible) face_visible[(int64_t)b * F + f] = 1;  // every writer stores the same byte
    }
    if (pix_to_face) pix_to_face[i] = face;
    if (zbuf) zbuf[i] = z;
    if (bary) {
        bary[3 * i] = b0;
        bary[3 * i + 1] = b1;
        bary[3 * i + 2] = b2;
    }
}

__global__ void __launch_bounds__(256) k_mesh_texels(int B, int F, int N, const uint8_t* __restrict__ face_visible,
                                                     const int32_t* __restrict__ binding_face,
                                                     uint8_t* __restrict__ texel_visible) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * N) return;
    const int b = (int)(i / N);
    const int f = binding_face[i - (int64_t)b * N];
    texel_visible[i] = (unsigned)f < (unsigned)F ? face_visible[(int64_t)b * F + f] : (uint8_t)0;
}

static unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_mesh_raster_workspace_bytes(int B, int V, int F, int W, int H) {
    if (!mesh_sizes_ok(B, V, F, W, H)) return 0;
    return mesh_layout(nullptr, B, V, F, W, H).bytes;
}

int gsr_mesh_raster(int B, int V, int F, int W, int H, const float* verts, const int32_t* faces, const float* w2c,
                    const float* tanfovx, const float* tanfovy, int packed, int32_t* pix_to_face, float* zbuf,
                    float* bary, uint8_t* face_visible, void* workspace, void* stream) {
    if (!mesh_sizes_ok(B, V, F, W, H)) return api_fail(GSR_ERR_ARG, "gsr_mesh_raster: bad sizes");
    if (!verts || !faces || !w2c || !tanfovx || !tanfovy || !workspace)
        return api_fail(GSR_ERR_ARG, "gsr_mesh_raster: null required pointer");
    const MeshLayout l = mesh_layout(workspace, B, V, F, W, H);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nv = (int64_t)B * V, nf = (int64_t)B * F, np = (int64_t)B * H * W;
    int64_t n0 = nv > np ? (nv > nf ? nv : nf) : (np > nf ? np : nf);  // k_mesh_project also resets the state
    if (n0 < kHeadWords) n0 = kHeadWords;
    hipLaunchKernelGGL(k_mesh_project, dim3(blocks256(n0)), dim3(256), 0, s, B, V, F, W, H, verts, w2c, tanfovx,
                       tanfovy, l.pv, l.keys, face_visible, l.head);
    hipLaunchKernelGGL(k_mesh_faces, dim3(blocks256(nf)), dim3(256), 0, s, B, V, F, W, H, faces, l.pv, l.keys,
                       l.worklist, l.head);
    const unsigned wide_blocks = (unsigned)((nf + 3) / 4 < kWideBlocks ? (nf + 3) / 4 : kWideBlocks);
    hipLaunchKernelGGL(k_mesh_faces_wide, dim3(wide_blocks), dim3(256), 0, s, B, V, F, W, H, faces, l.pv, l.keys,
                       l.worklist, l.head);
    hipLaunchKernelGGL(k_mesh_resolve, dim3(blocks256(np)), dim3(256), 0, s, B, V, F, W, H, packed, faces, l.pv,
                       l.keys, pix_to_face, zbuf, bary, face_visible, l.head);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

int gsr_mesh_visible_texels(int B, int F, int N, const uint8_t* face_visible, const int32_t* binding_face,
                            uint8_t* texel_visible, void* stream) {
    if (B <= 0 || F <= 0 || N <= 0 || (int64_t)B * N >= ((int64_t)1 << 31) || (int64_t)B * F >= ((int64_t)1 << 31))
        return api_fail(GSR_ERR_ARG, "gsr_mesh_visible_texels: bad sizes");
    if (!face_visible || !binding_face || !texel_visible)
        return api_fail(GSR_ERR_ARG, "gsr_mesh_visible_texels: null pointer");
    hipLaunchKernelGGL(k_mesh_texels, dim3(blocks256((int64_t)B * N)), dim3(256), 0, (hipStream_t)stream, B, F, N,
                       face_visible, binding_face, texel_visible);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

int gsr_mesh_raster_stats(const void* workspace, int64_t out[4]) {
    if (!workspace || !out) return api_fail(GSR_ERR_ARG, "gsr_mesh_raster_stats: null pointer");
    uint32_t h[kHeadWords];
    hipError_t e = hipMemcpy(h, workspace, sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return api_fail(GSR_ERR_HIP, hipGetErrorString(e));
    for (int k = 0; k < 4; ++k) {
        out[k] = 0;
        for (int sl = 0; sl < kStatSlots; ++sl) out[k] += (int64_t)h[16 + 16 * sl + k];
    }
    return 0;
}

}  // extern "C"
