// The loss and optimizer half of the training steps: everything that runs on NCHW fp32
// tensors and flat parameter buffers and uses none of the BatchNorm, weight-gradient or
// weight-pack code of train.hip.
//
//   chansum         deterministic per-channel sum of an NCHW fp32 tensor (bias grads)
//   softmax2        the 2-way softmax of fcams
//   tcam_losses     SelfLearningTcams CE(ignore -255) + ConRanFieldTcams + the ELB size
//                   term of MaxSizePositiveTcams (losses/tcam.py:48-278, elb.py:119-137),
//                   optionally BgSizeGreatSizeFgTcams, FgSizeTcams and EmptyOutsideBboxTcams
//                   (losses/tcam.py:281-430): forward values and d loss / d fcams through
//                   the 2-way softmax
//   teacher_stats   the dense box mask and fg_size of a batch of teacher CAMs
//   mosaic          RgbJointConRanFieldTcams' frame mosaics, gather and its adjoint
//   sgd_step        torch.optim.SGD(momentum, dampening, weight_decay, nesterov) step,
//                   plain, gated on the loss, or gated by the GradScaler as well
//   amp             torch.cuda.amp.GradScaler's unscale_ and update() on the device
#include "common.h"

namespace {

constexpr int kB = 256;

// ------------------------------------------------------------ chansum
__global__ __launch_bounds__(kB) void chansum_partial_kernel(const float* __restrict__ x,
                                                             int C, long HW, long chunk,
                                                             double* __restrict__ part,
                                                             int nchunks) {
    // grid (nchunks, B * C): sum over a chunk of one plane
    const long plane = blockIdx.y;
    const long h0 = (long)blockIdx.x * chunk, h1 = min(HW, h0 + chunk);
    double s = 0.0;
    for (long j = h0 + threadIdx.x; j < h1; j += kB) s += (double)x[plane * HW + j];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double red[kB / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kB / 64; ++i) t += red[i];
        part[plane * nchunks + blockIdx.x] = t;
    }
}

__global__ void chansum_final_kernel(const double* __restrict__ part, int B, int C, int nchunks,
                                     float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nchunks; ++k) s += part[((long)b * C + c) * nchunks + k];
    out[c] = (float)s;
}

// ------------------------------------------------------------- losses
// One kernel family, template <bool TERMS>: <false> is tcam_tcam_losses(_ex); <true>
// (tcam_tcam_losses_terms) adds BgSizeGreatSizeFgTcams, FgSizeTcams and EmptyOutsideBboxTcams
// (losses/tcam.py:281-430) under `if constexpr (TERMS)`, so with the three terms off every
// operation that feeds losses[0:5] and dfcams is the one of <false>, in the same order.
// Per-(frame, block) partials over pixels: sum S0, sum S1, CE sum, valid count, sum S.AS,
// and with TERMS sum S1 (1 - msk).
constexpr int kLossPix = 4096;

__device__ __forceinline__ void softmax2(float f0, float f1, float& s0, float& s1) {
    const float m = fmaxf(f0, f1);
    const float e0 = expf(f0 - m), e1 = expf(f1 - m);
    const float z = e0 + e1;
    s0 = e0 / z;
    s1 = e1 / z;
}

__global__ __launch_bounds__(kB) void softmax2_kernel(const float* __restrict__ f,
                                                      float* __restrict__ S, int B, long HW) {
    const long i = (long)blockIdx.x * kB + threadIdx.x;
    if (i >= (long)B * HW) return;
    const long b = i / HW, j = i - b * HW;
    float s0, s1;
    softmax2(f[(b * 2) * HW + j], f[(b * 2 + 1) * HW + j], s0, s1);
    S[(b * 2) * HW + j] = s0;
    S[(b * 2 + 1) * HW + j] = s1;
}

template <bool TERMS>
__global__ __launch_bounds__(kB) void loss_partial_kernel(
    const float* __restrict__ f, const float* __restrict__ S, const int32_t* __restrict__ seeds,
    const float* __restrict__ AS, const float* __restrict__ msk, long HW, int nchunks,
    double* __restrict__ part) {
    constexpr int NP = TERMS ? 6 : 5;
    const int b = blockIdx.y;
    const long j0 = (long)blockIdx.x * kLossPix, j1 = min(HW, j0 + kLossPix);
    double acc[NP] = {};   // S0, S1, CE, valid, S.AS (, S1 (1 - msk))
    for (long j = j0 + threadIdx.x; j < j1; j += kB) {
        const long o0 = (long)(b * 2) * HW + j, o1 = o0 + HW;
        const float s0 = S[o0], s1 = S[o1];
        acc[0] += s0;
        acc[1] += s1;
        if (seeds) {
            const int sd = seeds[(long)b * HW + j];
            if (sd == 0 || sd == 1) {
                // cross entropy = logsumexp(f) - f[seed]
                const float f0 = f[o0], f1 = f[o1];
                const float m = fmaxf(f0, f1);
                const float lse = m + logf(expf(f0 - m) + expf(f1 - m));
                acc[2] += (double)(lse - (sd ? f1 : f0));
                acc[3] += 1.0;
            }
        }
        if (AS) acc[4] += (double)s0 * AS[o0] + (double)s1 * AS[o1];
        if constexpr (TERMS)
            if (msk) acc[5] += (double)s1 * (1.0 - (double)msk[(long)b * HW + j]);
    }
    __shared__ double red[kB / 64][NP];
#pragma unroll
    for (int q = 0; q < NP; ++q)
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < NP; ++q) red[threadIdx.x >> 6][q] = acc[q];
    __syncthreads();
    if (threadIdx.x < NP) {
        double t = 0.0;
        for (int w = 0; w < kB / 64; ++w) t += red[w][threadIdx.x];
        part[((long)b * nchunks + blockIdx.x) * NP + threadIdx.x] = t;
    }
}

struct LossCfg {
    float lam_sl, lam_crf, lam_size, elb_t;
    int use_sl, use_crf, use_size;
};

struct TermsCfg {
    float lam_bgfg, lam_fgsz, lam_eob;   // 0 / NULL input: the term is off
    float t_bgfg, t_fgsz, t_eob;         // each term's own ELB t
    float eps;                           // FgSizeTcams.eps
    int use_bgfg, use_fgsz, use_eob;
};

// ELB.forward on one element, the fp32 formula of the size term below.  The size term does
// not call this: its threshold is (float)(-1.0 / (t * t)) rounded from fp64, which can differ
// from the fp32 quotient here by an ulp for t != 1.
__device__ __forceinline__ void elb_f32(float fx, float t, float& l, float& dl) {
    if (fx <= -1.f / (t * t)) {
        l = -(1.f / t) * logf(-fx);
        dl = -(1.f / t) / fx;
    } else {
        l = t * fx - (1.f / t) * logf(1.f / (t * t)) + 1.f / t;
        dl = t;
    }
}

// One block: the scalar losses and the per-frame gradient constants.
//   sl   = lam_sl * CE mean over valid seeds
//   crf  = lam_crf * -(sum S.AS) / B
//   size = lam_size * 0.5 * sum_c ELB(-sum_hw S_c)  (ELB mean over b, elb.py:119-137)
// and with TERMS (each ELB averaged over b, each barrier argument formed in fp64 from the
// fp64 plane sums and cast to fp32 once):
//   bgfg = lam * ELB(-(bg - fg)),  bg / fg = sum_hw S[b, 0 / 1]
//   fgsz = lam / 2 * (ELB(fs - eps - fg / HW) + ELB(fg / HW - fs - eps)),  fs = fg_size[b]
//   eob  = lam * ELB(sum_hw S[b, 1] (1 - msk[b]))
// coef: [0] = lam_sl / n_valid; [1] = the CRF factor; then CS = 2 (TERMS: 3) per frame:
// [2 + CS b + c] = the per-plane constant of d loss / d S[b, c, :] (size; TERMS: + bgfg +
// fgsz), and with TERMS [2 + 3b + 2] = the factor of (1 - msk) on plane 1 (eob).
// extra (optional): one more term's value already on the device (RgbJointConRanFieldTcams),
// added to the total and stored as losses[4].
// losses: {total, sl, crf, size} and [4] = extra when given; with TERMS all of
// losses[8] = {total, sl, crf, size, extra (0 without), bgfg, fgsz, eob}.
// Thread i takes frames i, i + 256, ... (its chunks in order), then thread 0 adds
// the 256 thread partials in order — a fixed summation order, so the result is
// deterministic (a single thread over B * nchunks dependent fp64 adds took ~0.6 ms at B = 256).
constexpr int kFinBlock = 256;
template <bool TERMS>
__global__ __launch_bounds__(kFinBlock) void loss_finalize_kernel(
    const double* __restrict__ part, int B, int nchunks, long HW, LossCfg cfg, TermsCfg tc,
    const float* __restrict__ fg_size, const float* __restrict__ extra,
    float* __restrict__ losses, float* __restrict__ coef) {
    constexpr int NP = TERMS ? 6 : 5, CS = TERMS ? 3 : 2;
    __shared__ double red[TERMS ? 7 : 4][kFinBlock];
    double ce = 0.0, nv = 0.0, sas = 0.0, size = 0.0, bgfg = 0.0, fgsz = 0.0, eob = 0.0;
    const double t = cfg.elb_t, ct = -1.0 / (t * t);
    for (int b = threadIdx.x; b < B; b += kFinBlock) {
        double bl[2] = {0.0, 0.0};
        double out = 0.0;
        for (int k = 0; k < nchunks; ++k) {
            const double* p = part + ((long)b * nchunks + k) * NP;
            bl[0] += p[0];
            bl[1] += p[1];
            ce += p[2];
            nv += p[3];
            sas += p[4];
            if constexpr (TERMS) out += p[5];
        }
        float cc[2], cm = 0.f;
        for (int c = 0; c < 2; ++c) {
            // ELB.forward on fx = -bl, elementwise (fx <= ct: -log(-fx)/t, else t fx - log(1/t^2)/t + 1/t)
            const float fx = (float)(-bl[c]);
            float l, dl;
            if (fx <= (float)ct) {
                l = -(1.f / (float)t) * logf(-fx);
                dl = -(1.f / (float)t) / fx;
            } else {
                l = (float)t * fx - (1.f / (float)t) * logf(1.f / ((float)t * (float)t)) +
                    1.f / (float)t;
                dl = (float)t;
            }
            size += (double)l;
            // loss = lam * 0.5 * sum_c mean_b ELB(fx);  d fx / d S = -1
            cc[c] = cfg.use_size ? -cfg.lam_size * 0.5f * dl / (float)B : 0.f;
        }
        if constexpr (TERMS) {
            if (tc.use_bgfg) {
                // fx = -(bg - fg): d fx / d S0 = -1, d fx / d S1 = +1
                float l, dl;
                elb_f32((float)(-(bl[0] - bl[1])), tc.t_bgfg, l, dl);
                bgfg += (double)l;
                const float g = tc.lam_bgfg * dl / (float)B;
                cc[0] -= g;
                cc[1] += g;
            }
            if (tc.use_fgsz) {
                // fx1 = fs - eps - fg / HW, fx2 = fg / HW - fs - eps: d / d S1 = -+ 1 / HW
                const double fg = bl[1] / (double)HW, fs = (double)fg_size[b];
                float l1, dl1, l2, dl2;
                elb_f32((float)(fs - (double)tc.eps - fg), tc.t_fgsz, l1, dl1);
                elb_f32((float)(fg - fs - (double)tc.eps), tc.t_fgsz, l2, dl2);
                fgsz += (double)l1 + (double)l2;
                cc[1] += tc.lam_fgsz * 0.5f * (dl2 - dl1) / ((float)B * (float)HW);
            }
            if (tc.use_eob) {
                float l, dl;
                elb_f32((float)out, tc.t_eob, l, dl);
                eob += (double)l;
                cm = tc.lam_eob * dl / (float)B;
            }
        }
        coef[2 + CS * b] = cc[0];
        coef[2 + CS * b + 1] = cc[1];
        if constexpr (TERMS) coef[2 + CS * b + 2] = cm;
    }
    red[0][threadIdx.x] = ce;
    red[1][threadIdx.x] = nv;
    red[2][threadIdx.x] = sas;
    red[3][threadIdx.x] = size;
    if constexpr (TERMS) {
        red[4][threadIdx.x] = bgfg;
        red[5][threadIdx.x] = fgsz;
        red[6][threadIdx.x] = eob;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    ce = nv = sas = size = bgfg = fgsz = eob = 0.0;
    for (int i = 0; i < kFinBlock; ++i) {
        ce += red[0][i];
        nv += red[1][i];
        sas += red[2][i];
        size += red[3][i];
        if constexpr (TERMS) {
            bgfg += red[4][i];
            fgsz += red[5][i];
            eob += red[6][i];
        }
    }
    // no valid seed in the whole batch: nn.CrossEntropyLoss(reduction="mean", ignore_index)
    // is 0 / 0 = NaN, and through the total it makes the gated SGD skip the step, as the
    // reference's isfinite(loss) check does (the gradient keeps no CE term: coef[0] = 0)
    float sl = 0.f;
    if (cfg.use_sl && nv > 0) sl = (float)(cfg.lam_sl * ce / nv);
    else if (cfg.use_sl && cfg.lam_sl != 0.f) sl = __builtin_nanf("");
    const float crf = cfg.use_crf ? (float)(cfg.lam_crf * -sas / B) : 0.f;
    const float sz = cfg.use_size ? (float)(cfg.lam_size * 0.5 * size / B) : 0.f;
    const float ex = extra ? extra[0] : 0.f;
    float total = extra ? ((sl + crf) + sz) + ex : (sl + crf) + sz;
    if constexpr (TERMS) {
        const float v_bgfg = tc.use_bgfg ? (float)((double)tc.lam_bgfg * bgfg / B) : 0.f;
        const float v_fgsz = tc.use_fgsz ? (float)((double)tc.lam_fgsz * 0.5 * fgsz / B) : 0.f;
        const float v_eob = tc.use_eob ? (float)((double)tc.lam_eob * eob / B) : 0.f;
        if (tc.use_bgfg) total += v_bgfg;
        if (tc.use_fgsz) total += v_fgsz;
        if (tc.use_eob) total += v_eob;
        losses[5] = v_bgfg;
        losses[6] = v_fgsz;
        losses[7] = v_eob;
    }
    losses[0] = total;
    losses[1] = sl;
    losses[2] = crf;
    losses[3] = sz;
    if (TERMS || extra) losses[4] = ex;
    coef[0] = (cfg.use_sl && nv > 0) ? (float)(cfg.lam_sl / nv) : 0.f;
    coef[1] = cfg.use_crf ? -2.f * cfg.lam_crf / (float)B : 0.f;
}

// d loss / d fcams per pixel:
//   gS_c = coef1 * AS_c + coef[2 + CS b + c] + gx_c   (CRF: -2 lam AS / B; the frame's
//                                               per-plane constant; gx: an extra term's
//                                               d loss / d S, or NULL)
//   gS_1 += coef[2 + 3b + 2] (1 - msk)          (TERMS: empty outside the box)
//   gf_c = S_c (gS_c - sum_j S_j gS_j)          (softmax backward)
//        + coef0 (S_c - [seed == c])            (CE, valid seeds only)
template <bool TERMS>
__global__ __launch_bounds__(kB) void loss_grad_kernel(
    const float* __restrict__ S, const int32_t* __restrict__ seeds, const float* __restrict__ AS,
    const float* __restrict__ gx, const float* __restrict__ msk, const float* __restrict__ coef,
    int B, long HW, float* __restrict__ gf) {
    constexpr int CS = TERMS ? 3 : 2;
    const long i = (long)blockIdx.x * kB + threadIdx.x;
    if (i >= (long)B * HW) return;
    const long b = i / HW, j = i - b * HW;
    const long o0 = (b * 2) * HW + j, o1 = o0 + HW;
    const float s0 = S[o0], s1 = S[o1];
    float g0 = coef[2 + CS * b], g1 = coef[2 + CS * b + 1];
    if (AS) {
        g0 += coef[1] * AS[o0];
        g1 += coef[1] * AS[o1];
    }
    if (gx) {
        g0 += gx[o0];
        g1 += gx[o1];
    }
    if constexpr (TERMS)
        if (msk) g1 += coef[2 + CS * b + 2] * (1.f - msk[b * HW + j]);
    const float dot = s0 * g0 + s1 * g1;
    float r0 = s0 * (g0 - dot), r1 = s1 * (g1 - dot);
    if (seeds) {
        const int sd = seeds[b * HW + j];
        if (sd == 0 || sd == 1) {
            r0 += coef[0] * (s0 - (sd == 0 ? 1.f : 0.f));
            r1 += coef[0] * (s1 - (sd == 1 ? 1.f : 0.f));
        }
    }
    gf[o0] = r0;
    gf[o1] = r1;
}

// The teacher's statistics of a batch of CAMs (train_wsol.py:792-842): the dense box mask
// msk (B, 1, H, W) = 1 inside bbox[b] = (x0, y0, x1, y1), rows y0..y1-1 and columns x0..x1-1,
// else 0, and fg_size[b] = sum(cam roi) / (H W) (fp64 sum, one block per frame, fixed order).
__global__ __launch_bounds__(kB) void teacher_stats_kernel(
    const float* __restrict__ cams, const uint8_t* __restrict__ roi,
    const int32_t* __restrict__ bbox, int H, int W, float* __restrict__ msk,
    float* __restrict__ fg_size) {
    const int b = blockIdx.x;
    const long HW = (long)H * W;
    const int x0 = bbox[4 * b], y0 = bbox[4 * b + 1], x1 = bbox[4 * b + 2], y1 = bbox[4 * b + 3];
    double s = 0.0;
    for (long j = threadIdx.x; j < HW; j += kB) {
        const int y = (int)(j / W), x = (int)(j - (long)y * W);
        msk[b * HW + j] = (y >= y0 && y < y1 && x >= x0 && x < x1) ? 1.f : 0.f;
        s += (double)cams[b * HW + j] * (double)roi[b * HW + j];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double red[kB / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kB / 64; ++i) t += red[i];
        fg_size[b] = (float)(t / (double)HW);
    }
}

// ------------------------------------------------- RgbJoint frame mosaics
// RgbJointConRanFieldTcams.pair_samples (losses/tcam.py:207-232): the frames of one group,
// in frame order, concatenated along the width.  idx (G, L): frame of group g at
// position p.  out (G, C, H, L*W) from src (B, C, H, W); 4 consecutive x per thread
// when W % 4 == 0 (16-B loads and stores), else one.
template <int V>
__global__ __launch_bounds__(kB) void mosaic_gather_kernel(const float* __restrict__ src,
                                                           const int32_t* __restrict__ idx,
                                                           int G, int L, int C, int H, int W,
                                                           float* __restrict__ out) {
    const int Wv = W / V;
    const long n = (long)G * L * C * H * Wv;
    const long i = (long)blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int xv = (int)(i % Wv);
    long r = i / Wv;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    r /= C;
    const int p = (int)(r % L);
    const int g = (int)(r / L);
    const int b = idx[g * L + p];
    const float* s = src + (((long)b * C + c) * H + y) * W + (long)xv * V;
    float* d = out + (((long)g * C + c) * H + y) * ((long)L * W) + (long)p * W + (long)xv * V;
    if constexpr (V == 4)
        *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s);
    else
        *d = *s;
}

// The adjoint: dst[b, c, y, x] (+)= coef * sum over the occurrences k of frame b (in
// occ[occ_start[b] .. occ_start[b+1]), each g * L + p, fixed order) of
// mosaic[g, c, y, p*W + x].  A frame repeated by _fill_minibatch sums its copies.
__global__ __launch_bounds__(kB) void mosaic_scatter_kernel(const float* __restrict__ mosaic,
                                                            const int32_t* __restrict__ occ_start,
                                                            const int32_t* __restrict__ occ,
                                                            int B, int L, int C, int H, int W,
                                                            float coef, int accumulate,
                                                            float* __restrict__ dst) {
    const long n = (long)B * C * H * W;
    const long i = (long)blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W);
    long r = i / W;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    const int k0 = occ_start[b], k1 = occ_start[b + 1];
    if (k0 == k1 && accumulate) return;
    float acc = 0.f;
    for (int k = k0; k < k1; ++k) {
        const int gp = occ[k], g = gp / L, p = gp - g * L;
        acc += mosaic[(((long)g * C + c) * H + y) * ((long)L * W) + (long)p * W + x];
    }
    dst[i] = accumulate ? dst[i] + coef * acc : coef * acc;
}

// ------------------------------------------------------------------ SGD
// torch.optim.SGD's update of element i; `first` initialises the momentum buffer (torch
// SGD's ``momentum_buffer is None``).
__device__ __forceinline__ void sgd_update(float* __restrict__ p, const float* __restrict__ g,
                                           float* __restrict__ buf, long i, float lr,
                                           float momentum, float dampening, float wd,
                                           int nesterov, bool first, float gscale) {
    float d = gscale == 1.f ? g[i] : g[i] * gscale;
    if (wd != 0.f) d = d + wd * p[i];
    if (momentum != 0.f) {
        float b;
        if (first)
            b = d;
        else
            b = momentum * buf[i] + (1.f - dampening) * d;
        buf[i] = b;
        d = nesterov ? d + momentum * b : b;
    }
    p[i] = p[i] - lr * d;
}

// What may skip the step on the device (no host sync; every rank reads the same all-reduced
// values):
//   None  nothing; the caller says which step is the first (gate, steps unused)
//   Loss  gate[0], the all-reduced loss, is not finite (learning/train_wsol.py:1181:
//         ``if loss.requires_grad and torch.isfinite(loss)``)
//   Amp   scaler.step + that gate: the loss is not finite OR a rank found a non-finite
//         gradient (gate[1] = found_inf summed over ranks != 0)
// With a gate, *steps counts the applied steps and the first applied one is the first.
enum class Gate { None, Loss, Amp };

template <Gate GATE>
__global__ __launch_bounds__(kB) void sgd_kernel(float* __restrict__ p,
                                                 const float* __restrict__ g,
                                                 float* __restrict__ buf, long n, float lr,
                                                 float momentum, float dampening, float wd,
                                                 int nesterov, int first, float gscale,
                                                 const float* __restrict__ gate,
                                                 const int* __restrict__ steps) {
    const long i = (long)blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    bool fst = first != 0;
    if constexpr (GATE != Gate::None) {
        if (!isfinite(gate[0])) return;
        if (GATE == Gate::Amp && gate[1] != 0.f) return;
        fst = *steps == 0;
    }
    sgd_update(p, g, buf, i, lr, momentum, dampening, wd, nesterov, fst, gscale);
}

__global__ void sgd_count_kernel(const float* __restrict__ gate, int* __restrict__ steps,
                                 int* __restrict__ skipped) {
    if (threadIdx.x == 0) {
        if (isfinite(*gate))
            steps[0] += 1;
        else if (skipped)
            skipped[0] += 1;
    }
}

// ------------------------------------------------------------------ AMP
// torch.cuda.amp.GradScaler on the device (learning/train_wsol.py:1077, 1180-1183:
// scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()).
// unscale_: g *= 1 / scale (a power of two: exact), found_inf = any non-finite g.
__global__ __launch_bounds__(kB) void amp_unscale_kernel(float* __restrict__ g, long n,
                                                         const float* __restrict__ scale,
                                                         float* __restrict__ found_inf) {
    const long i = (long)blockIdx.x * kB + threadIdx.x;
    const float inv = 1.0f / *scale;
    bool bad = false;
    if (i < n) {
        const float v = g[i];
        bad = !isfinite(v);
        g[i] = v * inv;
    }
    // one store per wave that saw a non-finite value (the flag only ever goes 0 -> 1)
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) *found_inf = 1.f;
}

// step counters + scaler.update(): a non-finite loss skips backward, step and update alike
// (train_wsol.py:1180); otherwise found_inf backs the scale off and resets the growth
// tracker, and growth_interval clean steps in a row grow it (torch GradScaler semantics)
__global__ void amp_update_kernel(const float* __restrict__ gate, int* __restrict__ steps,
                                  int* __restrict__ skipped, float* __restrict__ scale,
                                  int* __restrict__ tracker, float growth, float backoff,
                                  int interval) {
    if (threadIdx.x != 0) return;
    if (!isfinite(gate[0])) {
        if (skipped) skipped[0] += 1;
        return;
    }
    if (gate[1] != 0.f) {
        if (skipped) skipped[0] += 1;
        *scale = *scale * backoff;
        *tracker = 0;
        return;
    }
    steps[0] += 1;
    if (++*tracker >= interval) {
        *scale = *scale * growth;
        *tracker = 0;
    }
}

}  // namespace

// ================================================================== C ABI
extern "C" size_t tcam_chansum_ws_bytes(int B, int C, long HW) {
    const long chunk = 16384;
    const long nchunks = (HW + chunk - 1) / chunk;
    return (size_t)B * C * nchunks * sizeof(double);
}

extern "C" int tcam_chansum_nchw(const float* x, int B, int C, long HW, float* out, void* ws,
                                 void* stream) {
    TCAM_REQUIRE(x && out && ws && B > 0 && C > 0 && HW > 0);
    const long chunk = 16384;
    const int nchunks = (int)((HW + chunk - 1) / chunk);
    hipStream_t st = as_stream(stream);
    chansum_partial_kernel<<<dim3(nchunks, B * C), kB, 0, st>>>(x, C, HW, chunk, (double*)ws,
                                                                nchunks);
    TCAM_CHECK_LAUNCH();
    chansum_final_kernel<<<cdiv(C, 64), 64, 0, st>>>((const double*)ws, B, C, nchunks, out);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_softmax2(const float* fcams, float* S, int B, long HW, void* stream) {
    TCAM_REQUIRE(fcams && S && B > 0 && HW > 0);
    softmax2_kernel<<<cdiv((long)B * HW, kB), kB, 0, as_stream(stream)>>>(fcams, S, B, HW);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" size_t tcam_tcam_loss_ws_bytes(int B, long HW) {
    const long nchunks = (HW + kLossPix - 1) / kLossPix;
    return (size_t)B * nchunks * 5 * sizeof(double) + (size_t)(2 + 2 * B) * sizeof(float) + 256;
}

// The three launches of either family.  ws: B nchunks (TERMS ? 6 : 5) doubles, then coef.
template <bool TERMS>
static int tcam_losses_launch(const float* fcams, const float* S, const int32_t* seeds,
                              const float* AS, const float* gx, const float* extra,
                              const float* fg_size, const float* msk, int B, long HW,
                              float lam_sl, float lam_crf, float lam_size, float elb_t,
                              TermsCfg tc, float* losses, float* dfcams, void* ws,
                              void* stream) {
    hipStream_t st = as_stream(stream);
    const int nchunks = (int)((HW + kLossPix - 1) / kLossPix);
    double* part = (double*)ws;
    float* coef = (float*)((char*)ws + (size_t)B * nchunks * (TERMS ? 6 : 5) * sizeof(double));
    loss_partial_kernel<TERMS><<<dim3(nchunks, B), kB, 0, st>>>(fcams, S, seeds, AS, msk, HW,
                                                                nchunks, part);
    TCAM_CHECK_LAUNCH();
    LossCfg cfg{lam_sl, lam_crf, lam_size, elb_t, seeds != nullptr, AS != nullptr,
                lam_size != 0.f};
    loss_finalize_kernel<TERMS><<<1, kFinBlock, 0, st>>>(part, B, nchunks, HW, cfg, tc, fg_size,
                                                         extra, losses, coef);
    TCAM_CHECK_LAUNCH();
    loss_grad_kernel<TERMS><<<cdiv((long)B * HW, kB), kB, 0, st>>>(S, seeds, AS, gx, msk, coef,
                                                                    B, HW, dfcams);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_tcam_losses_ex(const float* fcams, const float* S, const int32_t* seeds,
                                   const float* AS, const float* gx, const float* extra,
                                   int B, long HW, float lam_sl, float lam_crf,
                                   float lam_size, float elb_t, float* losses, float* dfcams,
                                   void* ws, void* stream) {
    TCAM_REQUIRE(fcams && S && losses && dfcams && ws && B > 0 && HW > 0 && elb_t > 0.f);
    TCAM_REQUIRE((gx == nullptr) == (extra == nullptr));
    return tcam_losses_launch<false>(fcams, S, seeds, AS, gx, extra, nullptr, nullptr, B, HW,
                                     lam_sl, lam_crf, lam_size, elb_t, TermsCfg{}, losses,
                                     dfcams, ws, stream);
}

extern "C" int tcam_tcam_losses(const float* fcams, const float* S, const int32_t* seeds,
                                const float* AS, int B, long HW, float lam_sl, float lam_crf,
                                float lam_size, float elb_t, float* losses, float* dfcams,
                                void* ws, void* stream) {
    return tcam_tcam_losses_ex(fcams, S, seeds, AS, nullptr, nullptr, B, HW, lam_sl, lam_crf,
                               lam_size, elb_t, losses, dfcams, ws, stream);
}

extern "C" size_t tcam_tcam_loss_terms_ws_bytes(int B, long HW) {
    const long nchunks = (HW + kLossPix - 1) / kLossPix;
    return (size_t)B * nchunks * 6 * sizeof(double) + (size_t)(2 + 3 * B) * sizeof(float) + 256;
}

extern "C" int tcam_tcam_losses_terms(const float* fcams, const float* S, const int32_t* seeds,
                                      const float* AS, const float* gx, const float* extra,
                                      const float* fg_size, const float* msk, int B, long HW,
                                      float lam_sl, float lam_crf, float lam_size, float elb_t,
                                      float lam_bgfg, float lam_fgsz, float lam_eob,
                                      float t_bgfg, float t_fgsz, float t_eob, float eps,
                                      float* losses, float* dfcams, void* ws, void* stream) {
    TCAM_REQUIRE(fcams && S && losses && dfcams && ws && B > 0 && HW > 0 && elb_t > 0.f);
    TCAM_REQUIRE((gx == nullptr) == (extra == nullptr));
    TCAM_REQUIRE(t_bgfg > 0.f && t_fgsz > 0.f && t_eob > 0.f && eps >= 0.f);
    TermsCfg tc{lam_bgfg, lam_fgsz, lam_eob, t_bgfg, t_fgsz, t_eob, eps, lam_bgfg != 0.f,
                fg_size != nullptr && lam_fgsz != 0.f, msk != nullptr && lam_eob != 0.f};
    return tcam_losses_launch<true>(fcams, S, seeds, AS, gx, extra, fg_size,
                                    tc.use_eob ? msk : nullptr, B, HW, lam_sl, lam_crf, lam_size,
                                    elb_t, tc, losses, dfcams, ws, stream);
}

extern "C" int tcam_teacher_stats(const float* cams, const uint8_t* roi, const int32_t* bbox,
                                  int B, int H, int W, float* msk, float* fg_size,
                                  void* stream) {
    TCAM_REQUIRE(cams && roi && bbox && msk && fg_size && B > 0 && H > 0 && W > 0);
    teacher_stats_kernel<<<B, kB, 0, as_stream(stream)>>>(cams, roi, bbox, H, W, msk, fg_size);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_mosaic_gather(const float* src, const int32_t* idx, int G, int L, int C,
                                  int H, int W, float* out, void* stream) {
    TCAM_REQUIRE(src && idx && out && G > 0 && L > 0 && C > 0 && H > 0 && W > 0);
    hipStream_t st = as_stream(stream);
    if (W % 4 == 0) {
        const long n = (long)G * L * C * H * (W / 4);
        mosaic_gather_kernel<4><<<cdiv(n, kB), kB, 0, st>>>(src, idx, G, L, C, H, W, out);
    } else {
        const long n = (long)G * L * C * H * W;
        mosaic_gather_kernel<1><<<cdiv(n, kB), kB, 0, st>>>(src, idx, G, L, C, H, W, out);
    }
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_mosaic_scatter(const float* mosaic, const int32_t* occ_start,
                                   const int32_t* occ, int B, int L, int C, int H, int W,
                                   float coef, int accumulate, float* dst, void* stream) {
    TCAM_REQUIRE(mosaic && occ_start && occ && dst && B > 0 && L > 0 && C > 0 && H > 0 &&
                 W > 0);
    const long n = (long)B * C * H * W;
    mosaic_scatter_kernel<<<cdiv(n, kB), kB, 0, as_stream(stream)>>>(
        mosaic, occ_start, occ, B, L, C, H, W, coef, accumulate, dst);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_sgd_step(float* p, const float* g, float* buf, long n, float lr,
                             float momentum, float dampening, float weight_decay, int nesterov,
                             int first, float grad_scale, void* stream) {
    TCAM_REQUIRE(p && g && n > 0 && (momentum == 0.f || buf));
    sgd_kernel<Gate::None><<<cdiv(n, kB), kB, 0, as_stream(stream)>>>(
        p, g, buf, n, lr, momentum, dampening, weight_decay, nesterov, first, grad_scale, nullptr,
        nullptr);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_sgd_step_gated(float* p, const float* g, float* buf, long n, float lr,
                                   float momentum, float dampening, float weight_decay,
                                   int nesterov, float grad_scale, const float* gate,
                                   int* steps, int* skipped, void* stream) {
    TCAM_REQUIRE(p && g && gate && steps && n > 0 && (momentum == 0.f || buf));
    hipStream_t st = as_stream(stream);
    sgd_kernel<Gate::Loss><<<cdiv(n, kB), kB, 0, st>>>(p, g, buf, n, lr, momentum, dampening,
                                                       weight_decay, nesterov, 0, grad_scale,
                                                       gate, steps);
    TCAM_CHECK_LAUNCH();
    sgd_count_kernel<<<1, 64, 0, st>>>(gate, steps, skipped);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_amp_unscale(float* g, long n, const float* scale, float* found_inf,
                                void* stream) {
    TCAM_REQUIRE(g && scale && found_inf && n > 0);
    amp_unscale_kernel<<<cdiv(n, kB), kB, 0, as_stream(stream)>>>(g, n, scale, found_inf);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

extern "C" int tcam_sgd_step_amp(float* p, const float* g, float* buf, long n, float lr,
                                 float momentum, float dampening, float weight_decay,
                                 int nesterov, float grad_scale, const float* gate, int* steps,
                                 int* skipped, float* scale, int* tracker, float growth_factor,
                                 float backoff_factor, int growth_interval, void* stream) {
    TCAM_REQUIRE(p && g && gate && steps && scale && tracker && n > 0 &&
                 (momentum == 0.f || buf) && growth_interval > 0);
    hipStream_t st = as_stream(stream);
    sgd_kernel<Gate::Amp><<<cdiv(n, kB), kB, 0, st>>>(p, g, buf, n, lr, momentum, dampening,
                                                      weight_decay, nesterov, 0, grad_scale,
                                                      gate, steps);
    TCAM_CHECK_LAUNCH();
    amp_update_kernel<<<1, 64, 0, st>>>(gate, steps, skipped, scale, tracker, growth_factor,
                                        backoff_factor, growth_interval);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}
