// SSD training augmentation on the device: dn_augment_batch replaces, per batch, the reference's DetectionPresetTrain('ssd')
// (data/presets.py, data/transforms.py:30-239: RandomPhotometricDistort -> RandomZoomOut(fill = mean) -> RandomIoUCrop -> RandomHorizontalFlip ->
// ToTensor) AND the resize of the model's transform (transform.py:27-53,150-173) on the images: n decoded [h_i][w_i][3] uint8 images of any
// sizes -> one [n][3][out_h][out_w] fp32 batch in [0, 1], the input of dn_forward / SSD.loss. The random draws and the boxes are the host's
// (demonet_amd/augment.py); this file applies one parameter record per image (include/demonet_hip.h, DN_AUG_*).
//
// Semantics per image, x = u8 / 255 in fp32 (torchvision's tensor formulas):
//   gray(x) = 0.2989 r + 0.587 g + 0.114 b,   blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)
//   photometric, every step optional, in this order:
//     brightness  blend(x, 0, f)
//     contrast    blend(x, m, f), m = the mean of gray over the whole image AS IT STANDS at that point      [here when DN_AUG_F_CONTRAST_BEFORE]
//     saturation  blend(x, gray(x), f)
//     hue         rgb -> hsv (_rgb2hsv, with its maxc == minc guards), h = (h + f) mod 1, hsv -> rgb (_hsv2rgb: sector table, p q t clamped to [0, 1])
//     contrast                                                                                             [here otherwise]
//     channels    out[c] = in[perm[c]]
//   zoom-out: a canvas Hc x Wc with that image at (left, top) and fill[c] elsewhere (the fill is neither distorted nor permuted)
//   crop (cl, ct, cw, ch) of the canvas, horizontal flip of the crop, bilinear resize (align_corners = False) of the crop to out_h x out_w by the
//   arithmetic of resize_kernel (dense.hip).
// All geometric steps are index maps and the photometric ones are pointwise apart from the mean, so three launches (one when no image has contrast on) do all of it with no intermediate image:
//   augment_mean_kernel    images with contrast on: gray of every pixel after the steps in front of contrast, summed in double per fixed chunk with a
//                          fixed-shape tree; one partial per workgroup. No float atomics: the same bits on every run.
//   augment_finish_kernel  one thread per image with contrast on: adds the image's partials in index order, divides by the pixel count in double
//                          and leaves the fp32 mean in the image's table row -- once per image, not once per output workgroup.
//   augment_kernel         one thread per output pixel: computes the four resize taps in crop coordinates, maps each through flip -> crop ->
//                          canvas -> image, takes fill[c] or the photometric value of the source pixel
//                          (the whole chain once per tap, three channels from one 3-byte read), blends and writes the three planes.
// A workgroup belongs to one image, so the branches on a record's flags are uniform. Adjacent lanes take adjacent ox: their stores are consecutive
// floats and, for a down-scaling crop, their taps are neighbours in the source row. A tap is read only where it lies inside the h x w of `sizes`,
// whatever the record says. Compiled with -ffp-contract=off: one rounding per operation, as tests/augment_ref.py emulate_fp32 restates it.
// No inline asm, no atomics.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"

namespace {

constexpr int AUG_NT = 256;                 // threads per workgroup of the mean and the output kernel
constexpr int AUG_CHUNK = 4096;             // pixels per chunk of the mean launch: 16 per thread
constexpr int AUG_MAX_PARTS = 256;          // partials per image; an image of more chunks gives workgroup k the chunks k, k + 256, ...

struct AugImage {                           // one row of the device table, 128 bytes
    const unsigned char* img;
    int h, w;
    int nparts;                             // partials the mean launch writes for this image; 0: contrast off
    float mean;                             // written by augment_finish_kernel
    int32_t rec[DN_AUG_WORDS];
    int32_t reserved1[6];
};
static_assert(sizeof(AugImage) == 128, "AugImage is 128 bytes");

__device__ __forceinline__ float recf(const AugImage& im, int i) { return __int_as_float(im.rec[i]); }

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }
__device__ __forceinline__ float blend(float a, float b, float f, float f1) { return clamp01(f * a + f1 * b); }

__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float f) {
    // _rgb2hsv
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float div = eqc ? 1.f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    const float hr = maxc == r ? bc - gc : 0.f;
    const float hg = (maxc == g && maxc != r) ? (2.f + rc) - bc : 0.f;
    const float hb = (maxc != g && maxc != r) ? (4.f + gc) - rc : 0.f;
    float h = (hr + hg) + hb;
    h = fmodf(h / 6.f + 1.f, 1.f);
    // the shift, Python's float modulo: x - floor(x)
    h = h + f;
    h = h - floorf(h);
    // _hsv2rgb
    const float v = maxc;
    const float h6 = h * 6.f;
    const float fl = floorf(h6);
    const float fr = h6 - fl;
    int i = (int)fl;
    i = i >= 6 ? i - 6 : i;
    const float p = clamp01(v * (1.f - s));
    const float q = clamp01(v * (1.f - s * fr));
    const float t = clamp01(v * (1.f - s * (1.f - fr)));
    r = (i == 0 || i == 5) ? v : (i == 1 ? q : (i == 4 ? t : p));
    g = (i == 1 || i == 2) ? v : (i == 3 ? q : (i == 0 ? t : p));
    b = (i == 3 || i == 4) ? v : (i == 5 ? q : (i == 2 ? t : p));
}

// the steps in front of the second contrast position; `upto_contrast`: stop where the record's contrast step reads its mean
__device__ __forceinline__ void photo_front(const AugImage& im, int flags, float& r, float& g, float& b, float mean, bool upto_contrast) {
    if (flags & DN_AUG_F_BRIGHTNESS) {
        const float f = recf(im, DN_AUG_BRIGHTNESS);
        r = clamp01(f * r); g = clamp01(f * g); b = clamp01(f * b);
    }
    const bool contrast = (flags & DN_AUG_F_CONTRAST) != 0, before = (flags & DN_AUG_F_CONTRAST_BEFORE) != 0;
    if (contrast && before) {
        if (upto_contrast) return;
        const float f = recf(im, DN_AUG_CONTRAST), f1 = 1.f - f;
        r = blend(r, mean, f, f1); g = blend(g, mean, f, f1); b = blend(b, mean, f, f1);
    }
    if (flags & DN_AUG_F_SATURATION) {
        const float f = recf(im, DN_AUG_SATURATION), f1 = 1.f - f;
        const float y = gray_of(r, g, b);
        r = blend(r, y, f, f1); g = blend(g, y, f, f1); b = blend(b, y, f, f1);
    }
    if (flags & DN_AUG_F_HUE) hue_shift(r, g, b, recf(im, DN_AUG_HUE));
}

__device__ __forceinline__ void load_rgb(const unsigned char* p, float& r, float& g, float& b) {
    r = (float)p[0] / 255.f; g = (float)p[1] / 255.f; b = (float)p[2] / 255.f;
}

__global__ __launch_bounds__(AUG_NT) void augment_mean_kernel(const AugImage* __restrict__ tab, double* __restrict__ parts) {
    const AugImage& im = tab[blockIdx.y];
    if ((int)blockIdx.x >= im.nparts) return;
    __shared__ double sh[AUG_NT];
    const int flags = im.rec[DN_AUG_FLAGS];
    const long npix = (long)im.h * im.w;
    const long nchunks = (npix + AUG_CHUNK - 1) / AUG_CHUNK;
    double acc = 0.0;
    for (long chunk = blockIdx.x; chunk < nchunks; chunk += AUG_MAX_PARTS) {
#pragma unroll 4
        for (int j = 0; j < AUG_CHUNK / AUG_NT; ++j) {
            const long p = chunk * AUG_CHUNK + j * AUG_NT + threadIdx.x;
            if (p < npix) {
                float r, g, b;
                load_rgb(im.img + p * 3, r, g, b);
                photo_front(im, flags, r, g, b, 0.f, true);
                acc += (double)gray_of(r, g, b);
            }
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = AUG_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) parts[(size_t)blockIdx.y * AUG_MAX_PARTS + blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(64) void augment_finish_kernel(AugImage* __restrict__ tab, const double* __restrict__ parts, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int np = tab[i].nparts;
    if (np <= 0) return;
    double s = 0.0;
    const double* q = parts + (size_t)i * AUG_MAX_PARTS;
    for (int k = 0; k < np && k < AUG_MAX_PARTS; ++k) s += q[k];
    tab[i].mean = (float)(s / (double)((long)tab[i].h * tab[i].w));
}

__global__ __launch_bounds__(AUG_NT) void augment_kernel(const AugImage* __restrict__ tab, float* __restrict__ out, int oh, int ow) {
    const AugImage& im = tab[blockIdx.y];
    const int flags = im.rec[DN_AUG_FLAGS];
    const int idx = blockIdx.x * AUG_NT + threadIdx.x;
    if (idx >= oh * ow) return;
    const float mean = (flags & DN_AUG_F_CONTRAST) ? im.mean : 0.f;
    const int oy = idx / ow, ox = idx - oy * ow;
    const int h = im.h, w = im.w;
    const int left = im.rec[DN_AUG_LEFT], top = im.rec[DN_AUG_TOP];
    const int cl = im.rec[DN_AUG_CROP_L], ct = im.rec[DN_AUG_CROP_T], cw = im.rec[DN_AUG_CROP_W], ch = im.rec[DN_AUG_CROP_H];
    // the taps of resize_kernel (dense.hip), in crop coordinates
    const float rh = (float)ch / (float)oh, rw = (float)cw / (float)ow;
    const float sy = fmaxf(rh * ((float)oy + 0.5f) - 0.5f, 0.f);
    const float sx = fmaxf(rw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)sy, ch - 1), x0 = min((int)sx, cw - 1);
    const int y1 = y0 + (y0 < ch - 1 ? 1 : 0), x1 = x0 + (x0 < cw - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const bool flip = (flags & DN_AUG_F_FLIP) != 0;
    const bool contrast_after = (flags & DN_AUG_F_CONTRAST) && !(flags & DN_AUG_F_CONTRAST_BEFORE);
    const int p0 = im.rec[DN_AUG_PERM + 0], p1 = im.rec[DN_AUG_PERM + 1], p2 = im.rec[DN_AUG_PERM + 2];
    float v[4][3];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int ty = (t & 2) ? y1 : y0, tx = (t & 1) ? x1 : x0;
        // crop -> flipped crop -> canvas -> image; int64: a record the host check let through by mistake must still not wrap into the image
        const long ix = (long)(flip ? cw - 1 - tx : tx) + cl - left;
        const long iy = (long)ty + ct - top;
        if (ix >= 0 && ix < w && iy >= 0 && iy < h) {
            float c[3];
            load_rgb(im.img + ((size_t)iy * w + (size_t)ix) * 3, c[0], c[1], c[2]);
            photo_front(im, flags, c[0], c[1], c[2], mean, false);
            if (contrast_after) {
                const float f = recf(im, DN_AUG_CONTRAST), f1 = 1.f - f;
                c[0] = blend(c[0], mean, f, f1); c[1] = blend(c[1], mean, f, f1); c[2] = blend(c[2], mean, f, f1);
            }
            v[t][0] = p0 == 0 ? c[0] : (p0 == 1 ? c[1] : c[2]);
            v[t][1] = p1 == 0 ? c[0] : (p1 == 1 ? c[1] : c[2]);
            v[t][2] = p2 == 0 ? c[0] : (p2 == 1 ? c[1] : c[2]);
        } else {
            v[t][0] = recf(im, DN_AUG_FILL + 0); v[t][1] = recf(im, DN_AUG_FILL + 1); v[t][2] = recf(im, DN_AUG_FILL + 2);
        }
    }
    float* o = out + (size_t)blockIdx.y * 3 * oh * ow + idx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t0 = hx * v[0][c], t1 = lx * v[1][c], b0 = hx * v[2][c], b1 = lx * v[3][c];
        const float tp = t0 + t1, bt = b0 + b1;
        const float u = hy * tp, d = ly * bt;
        o[(size_t)c * oh * ow] = u + d;
    }
}

inline float word_f(const int32_t* rec, int i) {
    float f;
    memcpy(&f, rec + i, 4);
    return f;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) size_t dn_augment_workspace_bytes(int n) {
    if (n <= 0 || n > 65535) return 0;
    return (size_t)n * (sizeof(AugImage) + AUG_MAX_PARTS * sizeof(double));
}

extern "C" __attribute__((visibility("default"))) int dn_augment_batch(const uint8_t* const* images, const int32_t* sizes, const int32_t* params, int n,
                                                                      int out_h, int out_w, float* out, void* workspace, size_t workspace_bytes,
                                                                      void* stream) {
    DN_REQUIRE(images && sizes && params && out && workspace, "dn_augment_batch: null argument");
    DN_REQUIRE(n >= 1 && out_h >= 1 && out_w >= 1, "dn_augment_batch: bad sizes n=%d out_h=%d out_w=%d", n, out_h, out_w);
    if (n > 65535 || (long long)out_h * out_w > 0x7FFFFFFFll - AUG_NT) {
        dn_set_error("dn_augment_batch: n=%d above 65535, or an output of 2^31 pixels or more", n);
        return DN_E_UNSUPPORTED;
    }
    DN_REQUIRE((reinterpret_cast<size_t>(workspace) & 15) == 0 && (reinterpret_cast<size_t>(out) & 3) == 0, "dn_augment_batch: workspace not 16-byte aligned or out not 4-byte aligned");
    DN_REQUIRE(workspace_bytes >= dn_augment_workspace_bytes(n), "dn_augment_batch: workspace of %zu B, %zu B needed", workspace_bytes,
               dn_augment_workspace_bytes(n));
    std::vector<AugImage> tab((size_t)n);
    int max_parts = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t* r = params + (size_t)i * DN_AUG_WORDS;
        const int h = sizes[2 * i], w = sizes[2 * i + 1];
        DN_REQUIRE(images[i], "dn_augment_batch: image %d is a null pointer", i);
        DN_REQUIRE(h >= 1 && w >= 1, "dn_augment_batch: image %d has size %d x %d", i, h, w);
        if ((long long)h * w > 0x7FFFFFFFll / 4) {
            dn_set_error("dn_augment_batch: image %d of %d x %d has more than 2^29 pixels", i, h, w);
            return DN_E_UNSUPPORTED;
        }
        const int flags = r[DN_AUG_FLAGS];
        DN_REQUIRE((flags & ~DN_AUG_F_ALL) == 0, "dn_augment_batch: record %d has unknown flag bits 0x%x", i, flags);
        const int Hc = r[DN_AUG_CANVAS_H], Wc = r[DN_AUG_CANVAS_W], left = r[DN_AUG_LEFT], top = r[DN_AUG_TOP];
        DN_REQUIRE(Hc >= 1 && Wc >= 1 && left >= 0 && top >= 0 && (long long)left + w <= Wc && (long long)top + h <= Hc,
                   "dn_augment_batch: record %d places the %d x %d image at (left=%d, top=%d) outside its %d x %d canvas", i, h, w, left, top, Hc, Wc);
        const int cl = r[DN_AUG_CROP_L], ct = r[DN_AUG_CROP_T], cw = r[DN_AUG_CROP_W], ch = r[DN_AUG_CROP_H];
        DN_REQUIRE(cw >= 1 && ch >= 1 && cl >= 0 && ct >= 0 && (long long)cl + cw <= Wc && (long long)ct + ch <= Hc,
                   "dn_augment_batch: record %d has the crop (l=%d, t=%d, w=%d, h=%d), empty or outside the %d x %d canvas", i, cl, ct, cw, ch, Hc, Wc);
        int seen = 0;
        for (int c = 0; c < 3; ++c) {
            const int p = r[DN_AUG_PERM + c];
            DN_REQUIRE(p >= 0 && p <= 2, "dn_augment_batch: record %d: perm[%d] = %d", i, c, p);
            seen |= 1 << p;
        }
        DN_REQUIRE(seen == 7, "dn_augment_batch: record %d: perm is not a permutation of 0 1 2", i);
        const int fidx[7] = {DN_AUG_BRIGHTNESS, DN_AUG_CONTRAST, DN_AUG_SATURATION, DN_AUG_HUE, DN_AUG_FILL, DN_AUG_FILL + 1, DN_AUG_FILL + 2};
        for (int k = 0; k < 7; ++k) DN_REQUIRE(std::isfinite(word_f(r, fidx[k])), "dn_augment_batch: record %d: word %d is not a finite float", i, fidx[k]);
        AugImage& a = tab[i];
        memset(&a, 0, sizeof(a));
        a.img = images[i];
        a.h = h;
        a.w = w;
        if (flags & DN_AUG_F_CONTRAST) {
            const long long chunks = ((long long)h * w + AUG_CHUNK - 1) / AUG_CHUNK;
            a.nparts = (int)(chunks < AUG_MAX_PARTS ? chunks : AUG_MAX_PARTS);
        }
        max_parts = a.nparts > max_parts ? a.nparts : max_parts;
        memcpy(a.rec, r, sizeof(a.rec));
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    AugImage* tab_dev = reinterpret_cast<AugImage*>(workspace);
    double* parts = reinterpret_cast<double*>(tab_dev + n);
    // `tab` is this call's own pageable memory and dies with it: an event behind the copy, waited for after the launches are enqueued, holds
    // the call until the copy has read it, whatever way the runtime takes for a pageable source (staging, or pinning and DMA for a large table)
    hipEvent_t copied;
    DN_HIP_CHECK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
    hipError_t e = hipMemcpyAsync(tab_dev, tab.data(), tab.size() * sizeof(AugImage), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(copied, s);
    if (e == hipSuccess) {
        if (max_parts > 0) {
            hipLaunchKernelGGL(augment_mean_kernel, dim3(max_parts, n), dim3(AUG_NT), 0, s, tab_dev, parts);
            hipLaunchKernelGGL(augment_finish_kernel, dim3(dn_cdiv(n, 64)), dim3(64), 0, s, tab_dev, parts, n);
        }
        dn_note_kernel("augment_kernel");
        hipLaunchKernelGGL(augment_kernel, dim3(dn_cdiv((long)out_h * out_w, AUG_NT), n), dim3(AUG_NT), 0, s, tab_dev, out, out_h, out_w);
        e = hipGetLastError();
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(s);         // the event may not have been recorded while the copy is in flight
    const hipError_t waited = hipEventSynchronize(copied);      // also on an error path: the copy may be in flight
    (void)hipEventDestroy(copied);
    DN_HIP_CHECK(e);
    DN_HIP_CHECK(waited);
    return DN_OK;
}
