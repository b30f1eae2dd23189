// opental_amd/csrc/input.hip -- clip preparation on the device.
//
// Replaces the host-side tail of THUMOS_Dataset.__getitem__ (AFSD/common/thumos_dataset.py:246-262) and the transforms
// it calls (AFSD/common/videotransforms.py:44-124): temporal slice + zero padding to clip_length, random / centre crop,
// horizontal flip, uint8 -> float, (x / 255) * 2 - 1, and the (T,H,W,3) -> (3,T,H,W) transpose of load_video_data
// (thumos_dataset.py:136-137).  The reference does all of it in numpy per sample and ships a 28 MB fp32 clip to the
// GPU; here the uint8 frames (4x smaller) are uploaded and one launch writes the normalised batch.  The random crop
// offsets and flip decisions stay on the host (same `random` calls, see common/input_pipeline.py) and arrive as
// parameters, so results are reproducible against the reference bit for bit.
// HBM-bound: 3 bytes read + 12 bytes written per pixel.
#include "common.h"

namespace {

struct ClipParams {      // one per clip, device array
    long long frame0;    // element offset of this clip's first frame in the uint8 frame buffer
    int valid_t;         // frames available (the rest of the clip is zero BEFORE normalisation, i.e. -1.0 after it)
    int crop_i, crop_j;  // top-left corner of the crop in the source frame
    int flip;            // bit 0: mirror along W after cropping; bit 1: pad frames are 127.5 before normalisation (exactly
                         // 0.0 after it: the ActivityNet loader, AFSD/common/anet_dataset.py:226-229) instead of 0 (-1.0)
};

__global__ __launch_bounds__(256) void prepare_clips_kernel(const unsigned char* __restrict__ frames,
                                                            const ClipParams* __restrict__ params, float* __restrict__ out,
                                                            int T, int Hs, int Ws, int Ho, int Wo) {
    const int b = blockIdx.y;
    const ClipParams p = params[b];
    const int plane = Ho * Wo;
    const long long vol = (long long)T * plane;
    float* ob = out + (long long)b * 3 * vol;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < vol; idx += (long long)gridDim.x * 256) {
        const int t = (int)(idx / plane);
        const int r = (int)(idx - (long long)t * plane);
        const int y = r / Wo, x = r - y * Wo;
        float v0, v1, v2;
        if (t < p.valid_t) {
            const int xs = p.crop_j + ((p.flip & 1) ? Wo - 1 - x : x);
            const unsigned char* px = frames + p.frame0 + (((long long)t * Hs + (p.crop_i + y)) * Ws + xs) * 3;
            v0 = ((float)px[0] / 255.0f) * 2.0f - 1.0f;     // same operation order as the reference (no fma: -ffp-contract=off)
            v1 = ((float)px[1] / 255.0f) * 2.0f - 1.0f;
            v2 = ((float)px[2] / 255.0f) * 2.0f - 1.0f;
        } else {
            v0 = v1 = v2 = (((p.flip & 2) ? 127.5f : 0.0f) / 255.0f) * 2.0f - 1.0f;
        }
        ob[idx] = v0;
        ob[vol + idx] = v1;
        ob[2 * vol + idx] = v2;
    }
}

// The same preparation with an optional FRAME MAP per clip: output frame t is source frame map[t] of the (padded) clip.
// The self-supervised branch's spliced clip (thumos_dataset.py:187-228 `augment_`: two time segments of the normalised clip
// swap places) is exactly that, so one launch writes the plain batch and -- from the same uint8 upload and the same crop /
// flip decisions -- the ssl batch; the reference clones and slices a 28 MB fp32 clip per sample on the host.
__global__ __launch_bounds__(256) void prepare_clips_map_kernel(const unsigned char* __restrict__ frames,
                                                                const ClipParams* __restrict__ params,
                                                                const int* __restrict__ fmap, float* __restrict__ out,
                                                                float* __restrict__ out_ssl, int T, int Hs, int Ws, int Ho, int Wo) {
    const int b = blockIdx.y;
    const ClipParams p = params[b];
    const int plane = Ho * Wo;
    const long long vol = (long long)T * plane;
    for (int pass = 0; pass < 2; ++pass) {
        float* dst = pass == 0 ? out : out_ssl;
        if (!dst) continue;
        float* ob = dst + (long long)b * 3 * vol;
        for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < vol; idx += (long long)gridDim.x * 256) {
            const int t = (int)(idx / plane);
            const int r = (int)(idx - (long long)t * plane);
            const int y = r / Wo, x = r - y * Wo;
            const int ts = (pass == 1 && fmap) ? fmap[b * T + t] : t;
            float v0, v1, v2;
            if (ts >= 0 && ts < p.valid_t) {
                const int xs = p.crop_j + ((p.flip & 1) ? Wo - 1 - x : x);
                const unsigned char* px = frames + p.frame0 + (((long long)ts * Hs + (p.crop_i + y)) * Ws + xs) * 3;
                v0 = ((float)px[0] / 255.0f) * 2.0f - 1.0f;
                v1 = ((float)px[1] / 255.0f) * 2.0f - 1.0f;
                v2 = ((float)px[2] / 255.0f) * 2.0f - 1.0f;
            } else {
                v0 = v1 = v2 = (((p.flip & 2) ? 127.5f : 0.0f) / 255.0f) * 2.0f - 1.0f;
            }
            ob[idx] = v0;
            ob[vol + idx] = v1;
            ob[2 * vol + idx] = v2;
        }
    }
}

// The map kernel's preparation for CS source channels written as CO >= CS output planes (otal_prepare_clips_ch): planes
// c < CS are the normalised pixels, planes CS <= c < CO are +0.0f everywhere, padding frames included -- a 2-channel
// optical-flow clip becomes the 3-plane batch whose third plane the first layer multiplies with an all-zero weight slice.
// HBM-bound: CS bytes read + 4 CO written per pixel (flow: 2 + 12).  V pixels per thread: V = 4 where a crop row is a whole
// number of 16-byte groups (three 16-byte stores per thread, each wave instruction one contiguous 1 KB run per plane),
// V = 1 for any other shape (dword stores, coalesced along idx as in the kernels above).  A 2-channel pixel is ONE 16-bit
// load where the clip's first byte sits at an even address (every pixel offset is even; the same answer for a whole workgroup).
template <int CS>
__device__ __forceinline__ void load_pixel(const unsigned char* px, bool pair, float* v) {
    unsigned c0, c1, c2 = 0;
    if (CS == 2 && pair) {
        const unsigned w = *reinterpret_cast<const unsigned short*>(px);
        c0 = w & 0xffu;
        c1 = w >> 8;
    } else {
        c0 = px[0];
        c1 = px[1];
        if (CS == 3) c2 = px[2];
    }
    v[0] = ((float)c0 / 255.0f) * 2.0f - 1.0f;      // the operation order of the kernels above (no fma: -ffp-contract=off)
    v[1] = ((float)c1 / 255.0f) * 2.0f - 1.0f;
    if (CS == 3) v[2] = ((float)c2 / 255.0f) * 2.0f - 1.0f;
}

template <int CS, int CO, int V>
__global__ __launch_bounds__(256) void prepare_clips_ch_kernel(const unsigned char* __restrict__ frames,
                                                               const ClipParams* __restrict__ params,
                                                               const int* __restrict__ fmap, float* __restrict__ out,
                                                               float* __restrict__ out_ssl, int T, int Hs, int Ws, int Ho, int Wo) {
    static_assert(CS >= 2 && CS <= 3 && CO >= CS && CO <= 3 && (V == 1 || V == 4), "unsupported plane counts");
    const int b = blockIdx.y;
    const ClipParams p = params[b];
    const int plane = Ho * Wo;
    const long long vol = (long long)T * plane;
    const long long groups = vol / V;                   // V == 4 only with Wo % 4 == 0: a group never leaves its row
    const unsigned char* src = frames + p.frame0;
    const bool pair = (reinterpret_cast<unsigned long long>(src) & 1ull) == 0;
    const float pad = (((p.flip & 2) ? 127.5f : 0.0f) / 255.0f) * 2.0f - 1.0f;
    for (int pass = 0; pass < 2; ++pass) {
        float* dst = pass == 0 ? out : out_ssl;
        if (!dst) continue;
        float* ob = dst + (long long)b * CO * vol;
        for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
            const long long idx = gi * V;
            const int t = (int)(idx / plane);
            const int r = (int)(idx - (long long)t * plane);
            const int y = r / Wo, x = r - y * Wo;
            const int ts = (pass == 1 && fmap) ? fmap[b * T + t] : t;
            float v[V][3];
            if (ts >= 0 && ts < p.valid_t) {
                const unsigned char* row = src + (((long long)ts * Hs + (p.crop_i + y)) * Ws + p.crop_j) * CS;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int xo = (p.flip & 1) ? Wo - 1 - (x + j) : x + j;
                    load_pixel<CS>(row + xo * CS, pair, v[j]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) v[j][0] = v[j][1] = v[j][2] = pad;
            }
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                float* o = ob + c * vol + idx;
                if constexpr (V == 4) {
                    *reinterpret_cast<float4*>(o) = c < CS ? make_float4(v[0][c], v[1][c], v[2][c], v[3][c])
                                                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                } else {
                    *o = c < CS ? v[0][c] : 0.0f;
                }
            }
        }
    }
}

template <int CS, int CO>
int launch_prepare_clips_ch(const unsigned char* frames, const ClipParams* params, const int* frame_map, float* out,
                            float* out_ssl, int B, int T, int Hs, int Ws, int Ho, int Wo, hipStream_t stream) {
    const long long vol = (long long)T * Ho * Wo;
    const bool vec = Wo % 4 == 0 && ((reinterpret_cast<unsigned long long>(out) | reinterpret_cast<unsigned long long>(out_ssl)) & 15ull) == 0;
    const long long groups = vec ? vol / 4 : vol;
    // a streaming kernel: about eight workgroups per CU over the whole grid (256 CUs), the rest by grid stride
    const long long cap = 2048 / B > 0 ? 2048 / B : 1;
    const int bx = (int)((groups + 255) / 256 < cap ? (groups + 255) / 256 : cap);
    if (vec)
        hipLaunchKernelGGL((prepare_clips_ch_kernel<CS, CO, 4>), dim3(bx, B), dim3(256), 0, stream, frames, params, frame_map, out,
                           out_ssl, T, Hs, Ws, Ho, Wo);
    else
        hipLaunchKernelGGL((prepare_clips_ch_kernel<CS, CO, 1>), dim3(bx, B), dim3(256), 0, stream, frames, params, frame_map, out,
                           out_ssl, T, Hs, Ws, Ho, Wo);
    return otal_launch_status();
}

struct WindowParams {    // one per inference window, device array (16 bytes)
    unsigned long long src;  // device address of frame `offset` of channel 0 of the window's video (planar uint8 (C,Tv,H,W))
    int chan_stride4;        // Tv * H * W / 4: distance between the channels of that video, in 4-byte words
    int valid_t;             // frames available from `offset`; the rest of the window is 0.0 (zero padding AFTER normalisation)
};

// 4 pixels per thread: one dword load, one 16-byte store
__global__ __launch_bounds__(256) void prepare_windows_kernel(const WindowParams* __restrict__ params, float4* __restrict__ out,
                                                              int C, int T, int plane4) {
    const int b = blockIdx.y;
    const WindowParams p = params[b];
    const long long vol4 = (long long)T * plane4;
    const unsigned* src = reinterpret_cast<const unsigned*>(p.src);
    const long long valid4 = (long long)p.valid_t * plane4;
    for (int c = 0; c < C; ++c) {
        float4* ob = out + ((long long)b * C + c) * vol4;
        const unsigned* sc = src + (long long)c * p.chan_stride4;
        for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < vol4; idx += (long long)gridDim.x * 256) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < valid4) {
                const unsigned w = sc[idx];
                // the reference normalises the windows ON THE GPU (test.py:67-76 on a cuda tensor), where torch divides by a
                // scalar as a multiplication by its fp32 reciprocal -- unlike the training transforms, which run in numpy
                const float inv = 1.0f / 255.0f;
                v.x = ((float)(w & 0xffu) * inv) * 2.0f - 1.0f;
                v.y = ((float)((w >> 8) & 0xffu) * inv) * 2.0f - 1.0f;
                v.z = ((float)((w >> 16) & 0xffu) * inv) * 2.0f - 1.0f;
                v.w = ((float)(w >> 24) * inv) * 2.0f - 1.0f;
            }
            ob[idx] = v;
        }
    }
}

}  // namespace

extern "C" int otal_prepare_windows(const void* params, float* out, int B, int C, int T, int H, int W, void* stream) {
    if (!params || !out) return OTAL_E_NULL;
    if (B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0) return OTAL_E_SHAPE;
    if (B > 65535 || ((long long)H * W) % 4) return OTAL_E_UNSUPPORTED;
    const int plane4 = H * W / 4;
    const long long vol4 = (long long)T * plane4;
    const int bx = (int)((vol4 + 255) / 256 < 2048 ? (vol4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(prepare_windows_kernel, dim3(bx, B), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const WindowParams*>(params), reinterpret_cast<float4*>(out), C, T, plane4);
    return otal_launch_status();
}

extern "C" int otal_prepare_clips(const unsigned char* frames, const void* params, float* out, int B, int T, int Hs,
                                  int Ws, int Ho, int Wo, void* stream) {
    if (!frames || !params || !out) return OTAL_E_NULL;
    if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0 || Ho > Hs || Wo > Ws) return OTAL_E_SHAPE;
    if (B > 65535) return OTAL_E_UNSUPPORTED;
    const long long vol = (long long)T * Ho * Wo;
    const int bx = (int)((vol + 255) / 256 < 4096 ? (vol + 255) / 256 : 4096);
    hipLaunchKernelGGL(prepare_clips_kernel, dim3(bx, B), dim3(256), 0, (hipStream_t)stream, frames,
                       static_cast<const ClipParams*>(params), out, T, Hs, Ws, Ho, Wo);
    return otal_launch_status();
}

extern "C" int otal_prepare_clips_map(const unsigned char* frames, const void* params, const int* frame_map, float* out,
                                      float* out_ssl, int B, int T, int Hs, int Ws, int Ho, int Wo, void* stream) {
    if (!frames || !params || (!out && !out_ssl)) return OTAL_E_NULL;
    if (out_ssl && !frame_map) return OTAL_E_NULL;
    if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0 || Ho > Hs || Wo > Ws) return OTAL_E_SHAPE;
    if (B > 65535) return OTAL_E_UNSUPPORTED;
    const long long vol = (long long)T * Ho * Wo;
    const int bx = (int)((vol + 255) / 256 < 4096 ? (vol + 255) / 256 : 4096);
    hipLaunchKernelGGL(prepare_clips_map_kernel, dim3(bx, B), dim3(256), 0, (hipStream_t)stream, frames,
                       static_cast<const ClipParams*>(params), frame_map, out, out_ssl, T, Hs, Ws, Ho, Wo);
    return otal_launch_status();
}

extern "C" int otal_prepare_clips_ch(const unsigned char* frames, const void* params, const int* frame_map, float* out,
                                     float* out_ssl, int B, int C_src, int C_out, int T, int Hs, int Ws, int Ho, int Wo,
                                     void* stream) {
    if (!frames || !params || (!out && !out_ssl)) return OTAL_E_NULL;
    if (out_ssl && !frame_map) return OTAL_E_NULL;
    if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0 || Ho > Hs || Wo > Ws) return OTAL_E_SHAPE;
    if (B > 65535 || C_src < 2 || C_src > 3 || C_out < C_src || C_out > 3) return OTAL_E_UNSUPPORTED;
    const ClipParams* cp = static_cast<const ClipParams*>(params);
    hipStream_t st = (hipStream_t)stream;
    if (C_src == 3) return launch_prepare_clips_ch<3, 3>(frames, cp, frame_map, out, out_ssl, B, T, Hs, Ws, Ho, Wo, st);
    if (C_out == 3) return launch_prepare_clips_ch<2, 3>(frames, cp, frame_map, out, out_ssl, B, T, Hs, Ws, Ho, Wo, st);
    return launch_prepare_clips_ch<2, 2>(frames, cp, frame_map, out, out_ssl, B, T, Hs, Ws, Ho, Wo, st);
}
