// How a pixel of a video surface becomes three float values, and how four of them blend: the one definition shared by the network-input kernels of
// dense.hip (dn_forward_frames, dn_forward_regions) and the patch kernels of crops.hip (dn_crop_objects). include/demonet_hip.h fixes the arithmetic;
// both users must produce the same bits, which is why neither keeps a copy of its own.
#pragma once
#include "common.h"

// one rounding per operation, no FMA contraction: the float and the uint8 input paths must produce the same resized image
__device__ __forceinline__ float bilerp(float a, float b, float c, float d, float hx, float lx, float hy, float ly) {
#pragma clang fp contract(off)
    const float t0 = hx * a, t1 = lx * b, b0 = hx * c, b1 = lx * d;
    const float top = t0 + t1, bot = b0 + b1;
    const float u = hy * top, v = ly * bot;
    return u + v;
}

// Video surfaces (dn_forward_frames, include/demonet_hip.h): one dn_frame record per image, read from DEVICE memory at run time, every image
// with its own planes, pitches and size. A tap is converted to 8-bit RGB in integer arithmetic as it is read (1 luma + 2 chroma bytes; chroma
// sample (x >> 1, y >> 1)), then divided by 255 as u8hwc_kernel does.
struct FrameColor { int cy, crv, cbu, cgu, cgv, yo; };       // round(c * 2^14), the luma offset (frame_color below)

__device__ __forceinline__ int frame_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the 8-bit R, G, B of frame pixel (x, y)
template <int FMT>
__device__ __forceinline__ void frame_tap_rgb8(const dn_frame& f, int x, int y, const FrameColor& k, int& r, int& g, int& b) {
    if (FMT == DN_FRAME_RGB24 || FMT == DN_FRAME_BGR24) {
        const uint8_t* p = f.plane[0] + (size_t)y * f.pitch[0] + (size_t)x * 3;
        r = p[FMT == DN_FRAME_RGB24 ? 0 : 2]; g = p[1]; b = p[FMT == DN_FRAME_RGB24 ? 2 : 0];
    } else {
        const int yy = (int)f.plane[0][(size_t)y * f.pitch[0] + x] - k.yo;
        int u, v;
        if (FMT == DN_FRAME_NV12) {
            const uint8_t* p = f.plane[1] + (size_t)(y >> 1) * f.pitch[1] + (size_t)(x >> 1) * 2;
            u = (int)p[0] - 128; v = (int)p[1] - 128;
        } else {
            u = (int)f.plane[1][(size_t)(y >> 1) * f.pitch[1] + (x >> 1)] - 128;
            v = (int)f.plane[2][(size_t)(y >> 1) * f.pitch[2] + (x >> 1)] - 128;
        }
        const int l = k.cy * yy + (1 << 13);
        r = frame_clamp8((l + k.crv * v) >> 14);                    // >> of a signed int: arithmetic (floor)
        g = frame_clamp8((l - k.cgu * u - k.cgv * v) >> 14);
        b = frame_clamp8((l + k.cbu * u) >> 14);
    }
}

// ... and as the three floats the resize blends: x / 255 (ToTensor), a correctly rounded division. A kernel that keeps the 256 quotients in a table
// (crops.hip) fills it with this very expression.
__device__ __forceinline__ float frame_unit(int v) { return (float)v / 255.f; }

template <int FMT>
__device__ __forceinline__ void frame_tap(const dn_frame& f, int x, int y, const FrameColor& k, float* rgb) {
    int r, g, b;
    frame_tap_rgb8<FMT>(f, x, y, k, r, g, b);
    rgb[0] = frame_unit(r); rgb[1] = frame_unit(g); rgb[2] = frame_unit(b);
}

// round(c * 2^14) of cy = 255/219, crv = 2(1 - Kr) cs, cbu = 2(1 - Kb) cs, cgu = 2 Kb (1 - Kb) / Kg cs, cgv = 2 Kr (1 - Kr) / Kg cs with
// cs = 255/224, yo = 16 (limited range) or cy = cs = 1, yo = 0 (full range); BT.601: Kr, Kb = 0.299, 0.114, BT.709: 0.2126, 0.0722
// (tests/frames_ref.py derives the same integers from Kr, Kb in float64)
static inline bool frame_color(int color, FrameColor* k) {
    const bool full = (color & DN_COLOR_FULL_RANGE) != 0;
    switch (color & ~DN_COLOR_FULL_RANGE) {
        case DN_COLOR_BT601: *k = full ? FrameColor{16384, 22970, 29032, 5638, 11700, 0} : FrameColor{19077, 26149, 33050, 6419, 13320, 16}; return true;
        case DN_COLOR_BT709: *k = full ? FrameColor{16384, 25802, 30402, 3069, 7670, 0} : FrameColor{19077, 29372, 34610, 3494, 8731, 16}; return true;
    }
    return false;
}
