// Frame preprocessing in front of the vision tower (include/blim.h: blim_preprocess_frames): PIL's 8-bit bicubic resize restated as two
// integer passes, then the normalisation as a table lookup.  The host builds the taps (blim_amd/vision.py: bicubic_tables) and the
// table (normalise_lut); nothing here rounds on its own, so the result equals the host path's bit for bit.
//
// Both kernels are bound by their byte traffic (at most ~100 MB per video of 16 frames at 720 x 1280): one thread per output pixel with its
// three channels, the lanes of a wave on neighbouring pixels of one row, no LDS, no scratch.
//   horizontal: a wave's lanes read overlapping tap windows of one input row (the row is read from HBM once, the overlap from L1 / L2) and
//               store 192 contiguous bytes;
//   vertical:   every lane of a block has the same taps (one output row per block: the bounds and coefficients are scalar loads), each tap reads
//               192 contiguous bytes per wave, and the three channel planes are written as 128 contiguous bytes per wave.
#include "common.hpp"
#include "../../include/blim.h"

#define PRE_MAX_DIM 8192
#define PRE_BLOCK 256          // 4 waves; S = 448 is 1.75 blocks per row
#define PRE_SHIFT 22           // PIL's PRECISION_BITS for 8-bit images (32 - 8 - 2)

__device__ __forceinline__ int pre_clip8(int acc) {
    const int v = acc >> PRE_SHIFT;          // arithmetic shift: a negative sum (bicubic undershoot) stays negative and clips to 0
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// in [rows, W, 3] -> out [rows, S, 3]; grid (rows, ceil(S / PRE_BLOCK))
__global__ void __launch_bounds__(PRE_BLOCK) pre_horizontal_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int W, int S,
                                                                   const int32_t* __restrict__ xb, const int32_t* __restrict__ xk, int xks) {
    const int x = blockIdx.y * PRE_BLOCK + threadIdx.x;
    if (x >= S) return;
    const int64_t row = blockIdx.x;
    int first = xb[2 * x], n = xb[2 * x + 1];
    first = first < 0 ? 0 : (first > W ? W : first);              // the host asserts first + n <= W; a table that broke it reads no byte outside the row
    n = n > xks ? xks : n;
    n = n > W - first ? W - first : n;
    const uint8_t* p = in + (row * W + first) * 3;
    const int32_t* k = xk + (int64_t)x * xks;
    int a0 = 1 << (PRE_SHIFT - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < n; ++i) {
        const int c = k[i];
        a0 += c * p[3 * i]; a1 += c * p[3 * i + 1]; a2 += c * p[3 * i + 2];
    }
    uint8_t* o = out + (row * S + x) * 3;
    o[0] = (uint8_t)pre_clip8(a0); o[1] = (uint8_t)pre_clip8(a1); o[2] = (uint8_t)pre_clip8(a2);
}

// in [T, H, S, 3] -> out [T, 3, S, S] through the table; yb == nullptr: H == S and the bytes pass unchanged.  grid (T * S, ceil(S / PRE_BLOCK))
__global__ void __launch_bounds__(PRE_BLOCK) pre_vertical_kernel(const uint8_t* __restrict__ in, uint16_t* __restrict__ out, int H, int S,
                                                                 const int32_t* __restrict__ yb, const int32_t* __restrict__ yk, int yks,
                                                                 const uint16_t* __restrict__ lut) {
    const int x = blockIdx.y * PRE_BLOCK + threadIdx.x;
    if (x >= S) return;
    const int t = blockIdx.x / S, y = blockIdx.x % S;
    const uint8_t* frame = in + (int64_t)t * H * S * 3;
    int v0, v1, v2;
    if (yb) {
        int first = yb[2 * y], n = yb[2 * y + 1];
        first = first < 0 ? 0 : (first > H ? H : first);
        n = n > yks ? yks : n;
        n = n > H - first ? H - first : n;
        const uint8_t* p = frame + ((int64_t)first * S + x) * 3;
        const int32_t* k = yk + (int64_t)y * yks;
        int a0 = 1 << (PRE_SHIFT - 1), a1 = a0, a2 = a0;
        for (int i = 0; i < n; ++i) {
            const int c = k[i];
            const uint8_t* q = p + (int64_t)i * S * 3;
            a0 += c * q[0]; a1 += c * q[1]; a2 += c * q[2];
        }
        v0 = pre_clip8(a0); v1 = pre_clip8(a1); v2 = pre_clip8(a2);
    } else {
        const uint8_t* q = frame + ((int64_t)y * S + x) * 3;
        v0 = q[0]; v1 = q[1]; v2 = q[2];
    }
    const int64_t plane = (int64_t)S * S;
    uint16_t* o = out + (int64_t)t * 3 * plane + (int64_t)y * S + x;
    o[0] = lut[v0]; o[plane] = lut[256 + v1]; o[2 * plane] = lut[512 + v2];
}

static bool pre_dims_ok(int32_t T, int32_t H, int32_t W, int32_t S) {
    return T >= 1 && H >= 1 && W >= 1 && S >= 1 && T <= PRE_MAX_DIM && H <= PRE_MAX_DIM && W <= PRE_MAX_DIM && S <= PRE_MAX_DIM;
}

extern "C" int64_t blim_preprocess_workspace_bytes(int32_t T, int32_t H, int32_t W, int32_t S) {
    if (!pre_dims_ok(T, H, W, S)) { blim_set_error("blim_preprocess_workspace_bytes: T, H, W, S must lie in 1 .. %d (got %d, %d, %d, %d)", PRE_MAX_DIM, T, H, W, S); return BLIM_ERR_ARG; }
    return W == S ? 0 : (int64_t)T * H * S * 3;
}

extern "C" int blim_preprocess_frames(const uint8_t* frames, int32_t T, int32_t H, int32_t W, int32_t S, const int32_t* xb, const int32_t* xk, int32_t xks,
                                      const int32_t* yb, const int32_t* yk, int32_t yks, const uint16_t* lut, void* out, void* workspace, void* stream) {
    if (!pre_dims_ok(T, H, W, S)) { blim_set_error("blim_preprocess_frames: T, H, W, S must lie in 1 .. %d (got %d, %d, %d, %d)", PRE_MAX_DIM, T, H, W, S); return BLIM_ERR_ARG; }
    if (!frames || !lut || !out) { blim_set_error("blim_preprocess_frames: frames, lut and out must not be null"); return BLIM_ERR_ARG; }
    const bool horizontal = W != S, vertical = H != S;
    if (horizontal && (!xb || !xk || !workspace)) { blim_set_error("blim_preprocess_frames: W = %d != S = %d: the horizontal pass needs xb, xk and the workspace", W, S); return BLIM_ERR_ARG; }
    if (horizontal && xks < 1) { blim_set_error("blim_preprocess_frames: xks = %d: the horizontal pass needs at least one tap", xks); return BLIM_ERR_ARG; }
    if (vertical && (!yb || !yk)) { blim_set_error("blim_preprocess_frames: H = %d != S = %d: the vertical pass needs yb and yk", H, S); return BLIM_ERR_ARG; }
    if (vertical && yks < 1) { blim_set_error("blim_preprocess_frames: yks = %d: the vertical pass needs at least one tap", yks); return BLIM_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const unsigned xblocks = (unsigned)((S + PRE_BLOCK - 1) / PRE_BLOCK);
    const uint8_t* mid = frames;
    if (horizontal) {
        hipLaunchKernelGGL(pre_horizontal_kernel, dim3((unsigned)((int64_t)T * H), xblocks), dim3(PRE_BLOCK), 0, s, frames, (uint8_t*)workspace, (int)W, (int)S, xb, xk, (int)xks);
        mid = (const uint8_t*)workspace;
    }
    hipLaunchKernelGGL(pre_vertical_kernel, dim3((unsigned)((int64_t)T * S), xblocks), dim3(PRE_BLOCK), 0, s, mid, (uint16_t*)out, (int)H, (int)S,
                       vertical ? yb : nullptr, vertical ? yk : nullptr, (int)yks, lut);
    HIP_TRY(hipGetLastError());
    return BLIM_OK;
}
