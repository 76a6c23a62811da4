// Training-step kernels of the VGG16 (WSOL16) classifier (stage 1, task STD_CL with
// --encoder_name vgg16 --freeze_encoder False; encoders/vgg.py:61-161).  Its convolutions,
// pools, head, weight / data gradients and optimiser are the kernels the ResNet50 step uses
// (conv_x6.hip, pool.hip, train.hip, enc_train.hip).  This file adds what a BatchNorm-less
// conv + bias + ReLU stack with MaxPool2d(2, 2) needs:
//
//   relu_bwd        dz = dout [out > 0] (out: the saved post-ReLU activation), the bias
//                   gradient db[c] = sum_p dz[p, c] (fixed order: deterministic) and the
//                   per-channel max |dz| that tcam_dy_scaled_s2(compute = 0) turns into the
//                   MFMA copy's scale
//   maxpool2x2_bwd  the gradient of each 2x2 window goes to its first maximum in (kh, kw)
//                   order, NaN wins (torch's max_pool2d rule), recomputed from the forward
//                   input; the windows do not overlap: no atomics, no workspace
//
// Every byte offset comes from vgg_train_addr.h, which a host program checks over the whole
// launch grid of both kernels (tests/host/vgg_addr_check.cpp).
#include "common.h"
#include "s3_util.h"
#include "vgg_train_addr.h"

using s3::G8;

namespace {

constexpr int kB = vt::kBlock;

// ------------------------------------------------------------------ relu_bwd
// LG: the gradients' layout (S3 / S1), LA: the activation's (S2 / S1)
template <class LG, class LA>
__global__ __launch_bounds__(kB) void relu_bwd_kernel(const uint8_t* __restrict__ dout,
                                                      const uint8_t* __restrict__ out,
                                                      uint8_t* __restrict__ dz,
                                                      uint8_t* __restrict__ part,
                                                      uint32_t* __restrict__ amax,
                                                      vt::ReluGeom q) {
    __shared__ double ssum[kB * 8];
    __shared__ float smax[kB * 8];
    const int tid = threadIdx.x;
    const vt::ReluThread t = vt::relu_thread(q, blockIdx.x, tid);
    float s[8], m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = m[e] = 0.f;
    if (t.p0 >= 0) {
        for (long p = t.p0; p < q.P; p += t.step) {
            const G8 d = LG::load(dout + vt::group_off(p, q.G, t.g, LG::GB));
            const G8 a = LA::load(out + vt::group_off(p, q.G, t.g, LA::GB));
            G8 z;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                z.v[e] = a.v[e] > 0.f ? d.v[e] : 0.f;   // a copy or 0: exact in LG
                s[e] += z.v[e];
                m[e] = fmaxf(m[e], fabsf(z.v[e]));
            }
            LG::store(dz + vt::group_off(p, q.G, t.g, LG::GB), z);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        ssum[tid * 8 + e] = (double)s[e];
        smax[tid * 8 + e] = m[e];
    }
    __syncthreads();
    // rows 0 .. per - 1 of each channel in order (C may exceed the block: a strided loop)
    for (int c = tid; c < q.G * 8; c += kB) {
        double acc = 0.0;
        float mx = 0.f;
        for (int r = 0; r < q.per; ++r) {
            acc += ssum[vt::relu_lds_slot(q, r, c)];
            mx = fmaxf(mx, smax[vt::relu_lds_slot(q, r, c)]);
        }
        *reinterpret_cast<double*>(part + vt::relu_part_off(q, blockIdx.x, c)) = acc;
        // (the bit patterns of non-negative floats order as the values)
        if (amax && mx > 0.f) atomicMax(&amax[c], __float_as_uint(mx));
    }
}

// db[c] = the blocks' partial sums in block order; R16 (AMP): rounded to fp16, as an
// autocast conv's bias gradient
template <bool R16>
__global__ __launch_bounds__(kB) void relu_bwd_final_kernel(const uint8_t* __restrict__ part,
                                                            float* __restrict__ db,
                                                            vt::ReluGeom q) {
    const int c = blockIdx.x * kB + threadIdx.x;
    if (c >= q.G * 8) return;
    double acc = 0.0;
    for (int b = 0; b < q.blocks; ++b)
        acc += *reinterpret_cast<const double*>(part + vt::relu_part_off(q, b, c));
    float v = (float)acc;
    if (R16) v = (float)(_Float16)v;
    db[c] = v;
}

// ------------------------------------------------------------- maxpool2x2_bwd
template <class LG, class LA>
__global__ __launch_bounds__(kB) void maxpool2x2_bwd_kernel(const uint8_t* __restrict__ gout,
                                                            const uint8_t* __restrict__ x,
                                                            uint8_t* __restrict__ gin,
                                                            vt::PoolGeom q) {
    const long i = (long)blockIdx.x * kB + threadIdx.x;
    if (i >= q.total) return;
    const vt::PoolThread t = vt::pool_thread(q, i);
    G8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z.v[e] = 0.f;
    if (t.out_pix < 0) {   // a partial window of a last odd row / column: no output reads it
        for (int k = 0; k < 4; ++k)
            if (t.in_pix[k] >= 0) LG::store(gin + vt::group_off(t.in_pix[k], q.G, t.g, LG::GB), z);
        return;
    }
    // torch's max_pool2d: maxval = -inf, maxindex = the first tap; every tap in (kh, kw) order
    // replaces when (val > maxval || isnan(val))
    float best[8];
    int arg[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        best[e] = -INFINITY;
        arg[e] = 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const G8 v = LA::load(x + vt::group_off(t.in_pix[k], q.G, t.g, LA::GB));
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (v.v[e] > best[e] || isnan(v.v[e])) {
                best[e] = v.v[e];
                arg[e] = k;
            }
    }
    const G8 go = LG::load(gout + vt::group_off(t.out_pix, q.G, t.g, LG::GB));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) z.v[e] = arg[e] == k ? go.v[e] : 0.f;
        LG::store(gin + vt::group_off(t.in_pix[k], q.G, t.g, LG::GB), z);
    }
}

template <class LG, class LA, bool R16>
int relu_bwd(const void* dout, const void* out, void* dz, float* db, uint32_t* amax, long P,
             int C, void* ws, size_t ws_bytes, void* stream) {
    TCAM_REQUIRE(dout && out && dz && db && ws);
    TCAM_REQUIRE(dz != dout && dz != out);
    vt::ReluGeom q;
    TCAM_REQUIRE(vt::relu_geom(P, C, &q));
    TCAM_REQUIRE(ws_bytes >= vt::relu_ws_bytes(q));
    hipStream_t st = as_stream(stream);
    if (amax)
        TCAM_REQUIRE(hipMemsetAsync(amax, 0, (size_t)C * sizeof(uint32_t), st) == hipSuccess);
    relu_bwd_kernel<LG, LA><<<q.blocks, kB, 0, st>>>((const uint8_t*)dout, (const uint8_t*)out,
                                                     (uint8_t*)dz, (uint8_t*)ws, amax, q);
    TCAM_CHECK_LAUNCH();
    relu_bwd_final_kernel<R16><<<cdiv(C, kB), kB, 0, st>>>((const uint8_t*)ws, db, q);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

template <class LG, class LA>
int maxpool2x2_bwd(const void* gout, const void* x, void* gin, int B, int C, int H, int W, int Ho,
                   int Wo, void* stream) {
    TCAM_REQUIRE(gout && x && gin && gin != gout && gin != x);
    vt::PoolGeom q;
    TCAM_REQUIRE(vt::pool_geom(B, C, H, W, Ho, Wo, &q));
    const long nb = vt::blocks_for(q.total);
    TCAM_REQUIRE(nb <= 0x7fffffffl);
    maxpool2x2_bwd_kernel<LG, LA><<<(int)nb, kB, 0, as_stream(stream)>>>(
        (const uint8_t*)gout, (const uint8_t*)x, (uint8_t*)gin, q);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

}  // namespace

extern "C" size_t tcam_relu_bwd_ws_bytes(long P, int C) {
    vt::ReluGeom q;
    return vt::relu_geom(P, C, &q) ? vt::relu_ws_bytes(q) : 0;
}

extern "C" int tcam_relu_bwd_s3s2(const void* dout, const void* out, void* dz, float* db,
                                  uint32_t* amax, long P, int C, void* ws, size_t ws_bytes,
                                  void* stream) {
    return relu_bwd<LayS3, LayS2, false>(dout, out, dz, db, amax, P, C, ws, ws_bytes, stream);
}

extern "C" int tcam_relu_bwd_s1(const void* dout, const void* out, void* dz, float* db,
                                uint32_t* amax, long P, int C, void* ws, size_t ws_bytes,
                                void* stream) {
    return relu_bwd<LayS1, LayS1, true>(dout, out, dz, db, amax, P, C, ws, ws_bytes, stream);
}

extern "C" int tcam_maxpool2x2_bwd_s3s2(const void* gout, const void* x, void* gin, int B, int C,
                                        int H, int W, int Ho, int Wo, void* stream) {
    return maxpool2x2_bwd<LayS3, LayS2>(gout, x, gin, B, C, H, W, Ho, Wo, stream);
}

extern "C" int tcam_maxpool2x2_bwd_s1(const void* gout, const void* x, void* gin, int B, int C,
                                      int H, int W, int Ho, int Wo, void* stream) {
    return maxpool2x2_bwd<LayS1, LayS1>(gout, x, gin, B, C, H, W, Ho, Wo, stream);
}
