// CAM -> bbox on the GPU: a batched, exact replacement of
// compute_bboxes_from_scoremaps (metrics/wsol_metrics.py:127-197) with
// multi_contour_eval=False, i.e. for every threshold level L the box of
//   max(cv2.findContours(u8 > L, RETR_TREE, CHAIN_APPROX_SIMPLE), key=contourArea)
// followed by BoxEvaluator.accumulate (wsol_metrics.py:295-370).
//
// OpenCV semantics reproduced (contours.cpp, Suzuki-Abe border following on
// a zero-padded copy; contourArea = shoelace over the chain vertices):
//  * foreground is 8-connected, background 4-connected;
//  * the outer contour of a component C encloses C plus its holes, and its
//    shoelace area through pixel centres equals, summed over every 2x2
//    window of pixel centres, 1 if all four pixels lie in fill(C), 1/2 if
//    exactly three do, 0 otherwise;
//  * fill(C) of the top-level components are the 8-connected components of
//    {psi > L}, psi = grayscale hole-fill of u8 (min over 4-paths from the
//    image border of the max along the path);
//  * hole contours and contours nested in holes never win the max (strictly
//    smaller than their enclosing outer contour, and listed after it);
//  * ties between top-level contours resolve to the first in OpenCV's list
//    order = the LAST discovered in raster order = the largest raster index
//    of the component's first pixel;
//  * boundingRect of the outer contour = bbox of C.
// The oracle (oracle/contours.c, a restatement of the border follower) pins
// this characterisation on random images in tests/test_bbox_oracle.py.
//
// Two stages: the fill, one workgroup per frame (vmax = max(u8), psi, the
// histogram of psi -> the distinct levels: F_L only changes where psi = L + 1),
// and the level stage (the winning box of every distinct level).  Each has one
// production kernel per frame size and one independent reference, which
// tcam_bbox_fill_variant(1) / tcam_bbox_level_variant(1) select for the tests:
//
//   frame size   fill                            level stage
//   <= 224^2     fill_scan_kernel                level_sorted_kernel
//   <= 256^2     fill_scan_kernel                level_kernel<MAXH, MAXW, 2>
//   <= 320^2     fill_kernel<BIGH, BIGP, false>  level_kernel<BIGH, BIGW, 4>
//   reference    fill_kernel<MAXH, MAXP, true>   level_kernel
//
//  fill_scan_kernel     psi by row/column sweeps to the fixpoint, every line
//                       sweep a wave-parallel scan of composed clamps; also
//                       writes the psi-sorted pixel list of the sorted sweep.
//  fill_kernel          the same sweeps, one thread per line walking it in LDS;
//                       frames above 256^2 keep the u8 image in global memory
//                       so that psi alone fits in LDS.
//  level_sorted_kernel  walks a frame's levels from the top, adding each level's
//                       new pixels (a slice of the sorted list) to a union-find
//                       over 2x2 blocks whose roots carry area, first pixel and
//                       box; the winner is searched among the touched roots.
//  level_kernel         one workgroup per (frame, chunk of distinct levels), each
//                       level from scratch: psi in registers, per-level bitmap in
//                       LDS, block-based union-find (2x2 pixel blocks,
//                       8-connectivity), run-based window-area accumulation into
//                       root slots, argmax with OpenCV's tie order, bbox.
//  expand_kernel        copies each canonical level's box to the levels it stands
//                       for.
//  accumulate_kernel    one thread per (frame, tau): IoU vs GT (+1 inclusive
//                       convention, fp64) and the BoxEvaluator counters.
#include "common.h"

namespace {

constexpr int MAXH = 256, MAXW = 256;
constexpr int MAXP = 260;                 // padded row pitch in bytes (pitch_of(256))
constexpr int BIGH = 320, BIGW = 320;      // larger frames (299 x 299): psi-only LDS fill
constexpr int BIGP = 324;                  // pitch_of(320)
constexpr uint32_t INACT = 0xFFFFFFFFu;
constexpr int NTB = 1024;
constexpr int DBG_SLOTS = 16;   // per-workgroup phase-time slots (tcam_bbox_set_debug)
uint64_t* g_dbg = nullptr;
int g_fill_waves = NTB / 64;   // (debug) waves sweeping lines in fill_scan_kernel
int g_fill_maxit = 1 << 30;    // (debug) row + column passes at most
int g_fill_variant = 0;  // 0 = clamp-scan fill (default), 1 = LDS sweep fill (the cross-check)
int g_level_variant = 0;  // 0 = sorted-list sweep where it applies, 1 = level_kernel always
int g_bbox_chunks = 0;   // level ranges per frame for the next calls (0: the default)
uint64_t* g_inc_dbg = nullptr;  // per-WG phase ticks of level_sorted_kernel (profiling)

__device__ inline uint64_t rt() { return __builtin_amdgcn_s_memrealtime(); }
// Phase timer of the two level kernels (locals dbg, ph[8], tp): with a debug buffer, the ticks
// since the previous call are added to ph[k].
#define PHASE(k) do { if (dbg) { uint64_t t_ = rt(); ph[k] += t_ - tp; tp = t_; } } while (0)

__host__ __device__ inline int pitch_of(int W) {
    int d = (W + 3) / 4;
    if ((d & 1) == 0) d += 1;  // odd dword pitch: conflict-free column walks
    return 4 * d;
}

// Block-wide reductions over NTB threads (16 waves).
__device__ inline int block_max_i(int v, int* red) {
    v = wave_max_i(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = red[0];
        for (int i = 1; i < NTB / 64; ++i) m = max(m, red[i]);
        red[NTB / 64] = m;
    }
    __syncthreads();
    return red[NTB / 64];
}

// ------------------------------------------------------- sorted pixel list
// After the fill: the pixels with psi >= 1 listed by psi descending, for the sorted-list level
// sweep (level_sorted_kernel).  cgt[v] = #pixels with psi > v (v = 0..256); the pixels with
// psi == v sit at [cgt[v], cgt[v - 1]) as y << 8 | x, in no particular order (every quantity
// the sweep derives from a level's pixels is order-free: unions, sums, minima, maxima).
// hist (LDS, 257) holds the psi histogram; cur (LDS, 257) is scratch.  Called by every
// thread of the workgroup; wave 0 forms the suffix sums.
__device__ void emit_sorted(const uint8_t* psi, int P, const int* hist, int* cur, int H, int W,
                            int b, uint16_t* __restrict__ slist, int32_t* __restrict__ cgt) {
    const int tid = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    if (tid < 64) {
        // lane l owns the values u = 4l+1 .. 4l+4 (u <= 256; hist[256] = 0)
        int h[4], own = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            h[k] = hist[4 * tid + 1 + k];
            own += h[k];
        }
        int incl = own;   // suffix sum over lanes >= tid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(incl, o, 64);
            if (tid + o < 64) incl += t;
        }
        int above = incl - own;   // pixels with psi > 4l+4
        int32_t* cg = cgt + (long)b * 257;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            // cgt[4l + k] = above + hist[4l+k+1 .. 4l+4]
            above += h[k];
            cg[4 * tid + k] = above;
            cur[4 * tid + k] = above;
        }
        if (tid == 0) cg[256] = 0;
    }
    __syncthreads();
    uint16_t* out = slist + (long)b * H * W;
    for (int i = tid; i < H * W; i += nt) {
        const int y = i / W, x = i - y * W;
        const int v = psi[y * P + x];
        if (v) out[atomicAdd(&cur[v], 1)] = (uint16_t)(y << 8 | x);
    }
}

// ---------------------------------------------------------------- fill
// MH x MP: LDS plane geometry; IMG_LDS = false keeps the u8 image in global memory (L2)
// so frames up to 320 x 320 fit psi alone in LDS (InceptionV3 at 299, configs[4]).
template <int MH, int MP, bool IMG_LDS>
__global__ __launch_bounds__(NTB) void fill_kernel(const uint8_t* __restrict__ cam_u8,
                                                   uint8_t* __restrict__ psi_out,
                                                   int32_t* __restrict__ vmax_out,
                                                   int32_t* __restrict__ canon,
                                                   int32_t* __restrict__ lev_list,
                                                   int32_t* __restrict__ nlev, int H, int W,
                                                   uint64_t* __restrict__ dbg,
                                                   uint16_t* __restrict__ slist,
                                                   int32_t* __restrict__ cgt) {
    const uint64_t t0 = rt();
    __shared__ uint8_t img[IMG_LDS ? MH * MP : 4];
    __shared__ uint8_t psi[MH * MP];
    __shared__ int red[NTB / 64 + 1];
    __shared__ int hist[257];
    __shared__ int cur[257];
    __shared__ int changed;
    const int b = blockIdx.x;
    const int P = pitch_of(W);
    const uint8_t* src = cam_u8 + (long)b * H * W;
    int vm = 0;
    // 8 bytes per thread loaded together (a load-store loop waited on each load in turn)
    for (int i0 = threadIdx.x; i0 < H * W; i0 += 8 * NTB) {
        uint8_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * NTB;
            v[u] = i < H * W ? src[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * NTB;
            if (i >= H * W) continue;
            const int y = i / W, x = i - y * W;
            if (IMG_LDS) img[y * P + x] = v[u];
            psi[y * P + x] = 255;
            vm = max(vm, (int)v[u]);
        }
    }
    vm = block_max_i(vm, red);
    if (threadIdx.x == 0) vmax_out[b] = vm;
    const uint64_t t1 = rt();
    int iters = 0;
    // psi(p) = max(u8(p), min over 4-neighbours psi(q)), outside = -1.
    // Row sweeps (thread per row) alternate with column sweeps (thread per
    // column); each thread only reads/writes its own line, values only
    // decrease, and the loop stops after a full cycle without change.  The
    // sweeps are latency-bound chains, so rows are walked a dword (4 pixels)
    // at a time with the next dword prefetched, and columns 4 rows at a
    // time with the next 4 prefetched.
    const int nd = (W + 3) / 4;
    for (;;) {
        if (threadIdx.x == 0) changed = 0;
        __syncthreads();
        int ch = 0;
        if (threadIdx.x < H) {
            uint32_t* prow = reinterpret_cast<uint32_t*>(psi + threadIdx.x * P);
            const uint32_t* irow = reinterpret_cast<const uint32_t*>(img + threadIdx.x * P);
            const uint8_t* grow = src + threadIdx.x * W;
            auto idw = [&](int d) -> uint32_t {   // 4 pixels of the u8 row (0 past W)
                if (IMG_LDS) return irow[d];
                uint32_t v = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * d + e < W) v |= (uint32_t)grow[4 * d + e] << (8 * e);
                return v;
            };
            int prev = -1;
            uint32_t pv = prow[0], iv = idw(0);
            for (int d = 0; d < nd; ++d) {
                const uint32_t pn = d + 1 < nd ? prow[d + 1] : 0u;
                const uint32_t in = d + 1 < nd ? idw(d + 1) : 0u;
                uint32_t o = pv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (4 * d + e < W) {
                        const int c = (pv >> (8 * e)) & 255, u = (iv >> (8 * e)) & 255;
                        const int nv = max(u, min(c, prev));
                        prev = nv;
                        o = (o & ~(255u << (8 * e))) | ((uint32_t)nv << (8 * e));
                    }
                }
                if (o != pv) { prow[d] = o; ch = 1; }
                pv = pn;
                iv = in;
            }
            prev = -1;
            pv = prow[nd - 1];
            iv = idw(nd - 1);
            for (int d = nd - 1; d >= 0; --d) {
                const uint32_t pn = d > 0 ? prow[d - 1] : 0u;
                const uint32_t in = d > 0 ? idw(d - 1) : 0u;
                uint32_t o = pv;
#pragma unroll
                for (int e = 3; e >= 0; --e) {
                    if (4 * d + e < W) {
                        const int c = (pv >> (8 * e)) & 255, u = (iv >> (8 * e)) & 255;
                        const int nv = max(u, min(c, prev));
                        prev = nv;
                        o = (o & ~(255u << (8 * e))) | ((uint32_t)nv << (8 * e));
                    }
                }
                if (o != pv) { prow[d] = o; ch = 1; }
                pv = pn;
                iv = in;
            }
        }
        __syncthreads();
        if (threadIdx.x < W) {
            const int x = threadIdx.x;
            auto iat = [&](int y) -> int {
                return IMG_LDS ? (int)img[y * P + x] : (int)src[y * W + x];
            };
            // forward (down), 4 rows per group, next group prefetched
            int prev = -1;
            int c[4], u[4], cn[4], un[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c[e] = e < H ? psi[e * P + x] : 0;
                u[e] = e < H ? iat(e) : 0;
            }
            for (int y0 = 0; y0 < H; y0 += 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int y = y0 + 4 + e;
                    cn[e] = y < H ? psi[y * P + x] : 0;
                    un[e] = y < H ? iat(y) : 0;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int y = y0 + e;
                    if (y < H) {
                        const int nv = max(u[e], min(c[e], prev));
                        if (nv != c[e]) { psi[y * P + x] = (uint8_t)nv; ch = 1; }
                        prev = nv;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) { c[e] = cn[e]; u[e] = un[e]; }
            }
            // backward (up)
            prev = -1;
            const int top = ((H - 1) / 4) * 4;   // first row of the last group
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int y = top + e;
                c[e] = y < H ? psi[y * P + x] : 0;
                u[e] = y < H ? iat(y) : 0;
            }
            for (int y0 = top; y0 >= 0; y0 -= 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int y = y0 - 4 + e;
                    cn[e] = y >= 0 ? psi[y * P + x] : 0;
                    un[e] = y >= 0 ? iat(y) : 0;
                }
#pragma unroll
                for (int e = 3; e >= 0; --e) {
                    const int y = y0 + e;
                    if (y < H) {
                        const int nv = max(u[e], min(c[e], prev));
                        if (nv != c[e]) { psi[y * P + x] = (uint8_t)nv; ch = 1; }
                        prev = nv;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) { c[e] = cn[e]; u[e] = un[e]; }
            }
        }
        if (ch) changed = 1;  // benign same-value race
        __syncthreads();
        ++iters;
        if (!__builtin_amdgcn_readfirstlane(changed)) break;
        __syncthreads();
    }
    const uint64_t t2 = rt();
    uint8_t* dst = psi_out + (long)b * H * W;
    for (int i = threadIdx.x; i < 257; i += NTB) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < H * W; i += NTB) {
        int y = i / W, x = i - y * W;
        const uint8_t v = psi[y * P + x];
        dst[i] = v;
        atomicAdd(&hist[v], 1);
    }
    __syncthreads();
    // F_L = {psi > L} only changes at L = v - 1 for psi values v present:
    // compute boxes for those levels only; canon[L] names the level whose
    // F (and box) equals F_L (max(psi) = vmax, so every L < vmax maps).
    if (threadIdx.x == 0) {
        int n = 0, next = vm - 1;
        for (int L = vm - 1; L >= 0; --L) {
            if (hist[L + 1] > 0) next = L;
            canon[b * 256 + L] = next;
        }
        for (int L = 0; L < vm; ++L)
            if (hist[L + 1] > 0) lev_list[b * 256 + n++] = L;
        nlev[b] = n;
        if (dbg) {
            uint64_t* d = dbg + (long)b * DBG_SLOTS;
            d[0] = t1 - t0; d[1] = t2 - t1; d[2] = rt() - t2; d[3] = iters; d[4] = n;
        }
    }
    if (slist) emit_sorted(psi, P, hist, cur, H, W, b, slist, cgt);
}

// ------------------------------------------------------- fill (clamp scans)
// Same psi as fill_kernel, with every line sweep a wave-parallel scan.  A sweep step
// x_i = max(u_i, min(psi_i, x_{i-1})) clamps x_{i-1} to [u_i, psi_i] (psi >= u always), and
// clamps compose into clamps: clamp[a2,b2] o clamp[a1,b1] = clamp[c(a1), c(b1)] with
// c = clamp[a2,b2].  So a line of <= 256 pixels is 4 pixels per lane: each lane composes its
// 4 clamps, a 6-step shuffle scan composes the lanes' prefixes, and each lane replays its 4
// steps from its entry value (the lower end of the prefix clamp: what -1, the outside, maps
// to).  16 waves take a line each (rows, then columns) until a row + column pass changes
// nothing.  Pixels past the line end are u = psi = 0 (clamp[0,0]), which acts like the
// outside for the backward pass.  The histogram, the level tables and the psi-sorted pixel
// list (emit_sorted's output) follow in the same launch, wave-parallel.
constexpr int NTS = 1024;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

// DPP lane shifts (VALU, no LDS round trip): lanes whose source lies outside the row / wave
// get `old`.  Controls: row_shr:n = 0x110 + n, row_shl:n = 0x100 + n, wave_shr:1 = 0x138,
// wave_shl:1 = 0x130.
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v, int old) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xF, 0xF, false);
}

// compose the clamp [lo, hi] (applied second) after [plo, phi]
__device__ __forceinline__ void clamp_after(int& lo, int& hi, int plo, int phi) {
    const int nlo = clampi(plo, lo, hi), nhi = clampi(phi, lo, hi);
    lo = nlo;
    hi = nhi;
}

// forward (FWD: byte 0 -> 3, lane 0 -> 63) or backward sweep of the line held as one dword of
// psi (pw) and of u8 (uw) per lane.  In-row (16 lanes) Hillis-Steele scan over DPP row
// shifts; the rows' composites meet through readlane (scalar); the entry value of a lane is
// its predecessor's inclusive composite applied to -1, i.e. its lower end (wave shift by 1).
template <bool FWD>
__device__ __forceinline__ uint32_t scan_line4(uint32_t pw, uint32_t uw) {
    constexpr int IDLO = -1, IDHI = 256;   // the identity clamp
    int lo, hi;
    {
        constexpr int e0 = FWD ? 0 : 3;
        lo = (int)((uw >> (8 * e0)) & 255u);
        hi = (int)((pw >> (8 * e0)) & 255u);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const int e = FWD ? k : 3 - k;
            const int u = (int)((uw >> (8 * e)) & 255u), p = (int)((pw >> (8 * e)) & 255u);
            lo = clampi(lo, u, p);
            hi = clampi(hi, u, p);
        }
    }
    // in-row inclusive scan (sweep order)
#define SCAN_STEP(N)                                                                     \
    {                                                                                    \
        const int plo = FWD ? dpp_mov<0x110 + N>(lo, IDLO) : dpp_mov<0x100 + N>(lo, IDLO); \
        const int phi = FWD ? dpp_mov<0x110 + N>(hi, IDHI) : dpp_mov<0x100 + N>(hi, IDHI); \
        clamp_after(lo, hi, plo, phi);                                                   \
    }
    SCAN_STEP(1) SCAN_STEP(2) SCAN_STEP(4) SCAN_STEP(8)
#undef SCAN_STEP
    // rows: composites of the rows before this one in sweep order
    const int row = (int)(threadIdx.x & 63) >> 4;
    int qlo = IDLO, qhi = IDHI;
    if (FWD) {
        const int r0l = __builtin_amdgcn_readlane(lo, 15), r0h = __builtin_amdgcn_readlane(hi, 15);
        const int r1l = __builtin_amdgcn_readlane(lo, 31), r1h = __builtin_amdgcn_readlane(hi, 31);
        const int r2l = __builtin_amdgcn_readlane(lo, 47), r2h = __builtin_amdgcn_readlane(hi, 47);
        int q1l = r0l, q1h = r0h;                      // rows before row 1: row 0
        int q2l = r1l, q2h = r1h;
        clamp_after(q2l, q2h, q1l, q1h);               // rows 0..1
        int q3l = r2l, q3h = r2h;
        clamp_after(q3l, q3h, q2l, q2h);               // rows 0..2
        qlo = row == 1 ? q1l : row == 2 ? q2l : row == 3 ? q3l : IDLO;
        qhi = row == 1 ? q1h : row == 2 ? q2h : row == 3 ? q3h : IDHI;
    } else {
        const int s3l = __builtin_amdgcn_readlane(lo, 48), s3h = __builtin_amdgcn_readlane(hi, 48);
        const int s2l = __builtin_amdgcn_readlane(lo, 32), s2h = __builtin_amdgcn_readlane(hi, 32);
        const int s1l = __builtin_amdgcn_readlane(lo, 16), s1h = __builtin_amdgcn_readlane(hi, 16);
        int q2l = s3l, q2h = s3h;                      // rows after row 2: row 3
        int q1l = s2l, q1h = s2h;
        clamp_after(q1l, q1h, q2l, q2h);               // rows 3..2
        int q0l = s1l, q0h = s1h;
        clamp_after(q0l, q0h, q1l, q1h);               // rows 3..1
        qlo = row == 0 ? q0l : row == 1 ? q1l : row == 2 ? q2l : IDLO;
        qhi = row == 0 ? q0h : row == 1 ? q1h : row == 2 ? q2h : IDHI;
    }
    clamp_after(lo, hi, qlo, qhi);
    // entry: the predecessor's inclusive composite applied to -1 (its lower end)
    int x = FWD ? dpp_mov<0x138>(lo, -1) : dpp_mov<0x130>(lo, -1);
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = FWD ? k : 3 - k;
        const int u = (int)((uw >> (8 * e)) & 255u), p = (int)((pw >> (8 * e)) & 255u);
        x = max(u, min(p, x));
        out |= (uint32_t)x << (8 * e);
    }
    return out;
}

__global__ __launch_bounds__(NTS) void fill_scan_kernel(const uint8_t* __restrict__ cam_u8,
                                                        uint8_t* __restrict__ psi_out,
                                                        int32_t* __restrict__ vmax_out,
                                                        int32_t* __restrict__ canon,
                                                        int32_t* __restrict__ lev_list,
                                                        int32_t* __restrict__ nlev, int H, int W,
                                                        uint16_t* __restrict__ slist,
                                                        int32_t* __restrict__ cgt,
                                                        uint64_t* __restrict__ dbg, int nlw, int maxit) {
    const uint64_t t0 = rt();
    __shared__ uint8_t img[MAXH * MAXP];
    __shared__ uint8_t psi[MAXH * MAXP];
    __shared__ int red[NTS / 64];
    __shared__ int hist[257];
    __shared__ int cur[257];
    __shared__ int changed;
    const int b = blockIdx.x;
    // (wave id and the loop-exit flag are read into scalars: a loop whose exit the compiler
    // sees as per-lane is structurised into iterations with a partial exec mask, which the
    // cross-lane scans cannot tolerate)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = pitch_of(W);
    const int ndw = (W + 3) >> 2, ndh = (H + 3) >> 2;
    const uint8_t* src = cam_u8 + (long)b * H * W;
    int vm = 0;
    // rows of u8 and psi = 255 (0 in the padding bytes of the last dword)
    if ((W & 3) == 0 && ((uintptr_t)src & 3) == 0) {
        // whole dwords (a row is ndw of them, no padding), FILL_AHEAD per thread loaded
        // together: a byte load-store loop waited on each of its ~49 loads in turn
        constexpr int FILL_AHEAD = 4;
        const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
        const int nd = H * ndw;
        for (int i0 = tid; i0 < nd; i0 += FILL_AHEAD * NTS) {
            uint32_t v[FILL_AHEAD];
#pragma unroll
            for (int u = 0; u < FILL_AHEAD; ++u) {
                const int i = i0 + u * NTS;
                v[u] = i < nd ? src4[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < FILL_AHEAD; ++u) {
                const int i = i0 + u * NTS;
                if (i >= nd) continue;
                const int y = i / ndw, x4 = i - y * ndw;
                *reinterpret_cast<uint32_t*>(img + y * P + 4 * x4) = v[u];
                *reinterpret_cast<uint32_t*>(psi + y * P + 4 * x4) = 0xFFFFFFFFu;
                vm = max(vm, (int)max(max(v[u] & 255u, (v[u] >> 8) & 255u),
                                      max((v[u] >> 16) & 255u, v[u] >> 24)));
            }
        }
    } else {
        for (int i = tid; i < H * ndw * 4; i += NTS) {
            const int y = i / (ndw * 4), x = i - y * (ndw * 4);
            uint8_t v = 0;
            if (x < W) {
                v = src[y * W + x];
                vm = max(vm, (int)v);
            }
            img[y * P + x] = v;
            psi[y * P + x] = x < W ? 255 : 0;
        }
    }
    for (int i = tid; i < 257; i += NTS) hist[i] = 0;
    vm = wave_max_i(vm);
    if (lane == 0) red[wid] = vm;
    if (tid == 0) changed = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NTS / 64; ++i) vm = max(vm, red[i]);
    if (tid == 0) vmax_out[b] = vm;
    const uint64_t t1 = rt();
    int iters = 0;   // (scalar: block-uniform)

    for (;;) {
        bool ch = false;
        iters = __builtin_amdgcn_readfirstlane(iters + 1);
        for (int r = wid; r < H && wid < nlw; r += nlw) {
            uint32_t* prow = reinterpret_cast<uint32_t*>(psi + r * P);
            const uint32_t* irow = reinterpret_cast<const uint32_t*>(img + r * P);
            const bool in = lane < ndw;
            const uint32_t pw = in ? prow[lane] : 0u, uw = in ? irow[lane] : 0u;
            const uint32_t g = scan_line4<false>(scan_line4<true>(pw, uw), uw);
            if (in && g != pw) {
                prow[lane] = g;
                ch = true;
            }
        }
        __syncthreads();
        for (int c = wid; c < W && wid < nlw; c += nlw) {
            uint32_t pw = 0, uw = 0;
            if (lane < ndh) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int y = 4 * lane + e;
                    if (y < H) {
                        pw |= (uint32_t)psi[y * P + c] << (8 * e);
                        uw |= (uint32_t)img[y * P + c] << (8 * e);
                    }
                }
            }
            const uint32_t g = scan_line4<false>(scan_line4<true>(pw, uw), uw);
            if (lane < ndh && g != pw) {
                ch = true;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int y = 4 * lane + e;
                    if (y < H && ((g ^ pw) >> (8 * e)) & 255u) psi[y * P + c] = (uint8_t)(g >> (8 * e));
                }
            }
        }
        if (ch) changed = 1;  // benign same-value race
        __syncthreads();
        const int any = __builtin_amdgcn_readfirstlane(changed);
        __syncthreads();
        // (the reset precedes the exit test: a divergent if right before the latch of a loop
        // with an exit is structurised into a pass of lane 0 alone through the next
        // iteration — barriers and scans included)
        if (tid == 0) changed = 0;
        if (!any || iters >= maxit) break;
    }
    const uint64_t t2 = rt();

    // psi out + histogram (a wave whose 256 pixels share one value adds once)
    uint8_t* dst = psi_out + (long)b * H * W;
    for (int i = tid; i < H * W; i += NTS) {
        const int y = i / W, x = i - y * W;
        const int v = psi[y * P + x];
        dst[i] = (uint8_t)v;
        const int v0 = __shfl(v, 0, 64);
        const uint64_t act = __ballot(1);
        if (__ballot(v == v0) == act) {
            if (lane == 0) atomicAdd(&hist[v0], __popcll(act));
        } else {
            atomicAdd(&hist[v], 1);
        }
    }
    __syncthreads();
    // level tables (wave 0): lane l holds the levels L = 4l .. 4l+3 (present: hist[L+1] > 0)
    if (wid == 0) {
        int pres[4], np = 0, first = 256;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int L = 4 * lane + k;
            pres[k] = L < vm && hist[L + 1] > 0;
            np += pres[k];
        }
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (pres[k]) first = 4 * lane + k;
        // exclusive prefix of the counts (lev_list positions)
        int incl = np;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        int pos = incl - np;
        // smallest present level above this lane's range (suffix min over later lanes)
        int nxt = first;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(nxt, o, 64);
            if (lane + o < 64) nxt = min(nxt, t);
        }
        int above = __shfl_down(nxt, 1, 64);
        if (lane == 63) above = 256;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            const int L = 4 * lane + k;
            if (pres[k]) above = L;
            if (L < vm) canon[b * 256 + L] = above;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (pres[k]) lev_list[b * 256 + pos++] = 4 * lane + k;
        if (lane == 63) nlev[b] = incl;
    }
    const uint64_t t3 = rt();
    if (slist) emit_sorted(psi, P, hist, cur, H, W, b, slist, cgt);
    if (dbg && tid == 0) {
        uint64_t* d = dbg + (long)b * DBG_SLOTS;
        d[0] = t1 - t0; d[1] = t2 - t1; d[2] = t3 - t2; d[3] = iters; d[4] = rt() - t3;
    }
}

// one line through scan_line4 (tests): n <= 256 pixels, forward then (mode 0) backward
__global__ __launch_bounds__(64) void scan_line_kernel(const uint8_t* __restrict__ p,
                                                       const uint8_t* __restrict__ u,
                                                       uint8_t* __restrict__ out, int n, int mode) {
    const int lane = threadIdx.x;
    uint32_t pw = 0, uw = 0;
    for (int e = 0; e < 4; ++e) {
        const int x = 4 * lane + e;
        if (x < n) {
            pw |= (uint32_t)p[x] << (8 * e);
            uw |= (uint32_t)u[x] << (8 * e);
        }
    }
    uint32_t g = scan_line4<true>(pw, uw);
    if (mode == 0) g = scan_line4<false>(g, uw);
    for (int e = 0; e < 4; ++e) {
        const int x = 4 * lane + e;
        if (x < n) out[x] = (uint8_t)(g >> (8 * e));
    }
}

// --------------------------------------------------------------- levels
// One workgroup per (frame, chunk of distinct levels).  psi is held in
// registers (32 pixels = 8 packed dwords per bitmap word, <= 2 words per
// thread); each level builds the bitmap F = {psi > L} in LDS, labels 2x2
// pixel blocks with a lock-free union-find (atomicMin hooks toward the
// smaller index; in a 2x2 block all foreground pixels are 8-connected, so
// block labels are pixel labels), then reuses each ROOT's label slot as its
// area accumulator (flag bit 31 marks a root slot).
constexpr uint32_t RFLAG = 0x80000000u;
constexpr uint32_t NOKEY = RFLAG | 0x7FFFFFFFu;  // non-candidate root slot
constexpr int LEVEL_CHUNKS = 16;

__device__ inline uint32_t find_root(const volatile uint32_t* lab, uint32_t x) {
    uint32_t p = lab[x];
    while (p != x) {
        x = p;
        p = lab[x];
    }
    return x;
}

__device__ inline void unite(uint32_t* lab, uint32_t a, uint32_t b) {
    for (;;) {
        a = find_root(lab, a);
        b = find_root(lab, b);
        if (a == b) return;
        if (a > b) { uint32_t t = a; a = b; b = t; }
        uint32_t old = atomicMin(&lab[b], a);
        if (old == b) return;
        b = old;
    }
}

struct LevelCtx {
    const uint32_t* bm;  // bitmap, H x wpr words
    int H, W, wpr, BW;
    __device__ inline int bit(int y, int x) const {
        if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0;
        return (bm[y * wpr + (x >> 5)] >> (x & 31)) & 1;
    }
    // 2 bits (x, x+1) of row y, x even.
    __device__ inline int pair(int y, int x) const {
        if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0;
        return (bm[y * wpr + (x >> 5)] >> (x & 31)) & 3;
    }
    __device__ inline uint32_t word(int y, int j) const {
        if ((unsigned)y >= (unsigned)H || (unsigned)j >= (unsigned)wpr) return 0u;
        return bm[y * wpr + j];
    }
};

__device__ inline uint32_t root_of(const uint32_t* lab, uint32_t b) {
    uint32_t v = lab[b];
    return (v & RFLAG) ? b : v;
}

// LH x LW: largest frame; QW bitmap words (of 32 pixels) per thread.
template <int LH, int LW, int QW>
__global__ __launch_bounds__(NTB) void level_kernel(const uint8_t* __restrict__ psi_g,
                                                    const int32_t* __restrict__ vmax,
                                                    const int32_t* __restrict__ lev_list,
                                                    const int32_t* __restrict__ nlev,
                                                    int32_t* __restrict__ boxes, int H, int W,
                                                    uint64_t* __restrict__ dbg) {
    uint64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tp = rt();
    __shared__ uint32_t bm[LH * (LW / 32)];
    __shared__ uint32_t lab[(LH / 2) * (LW / 2)];
    __shared__ int red[4 * (NTB / 64) + 4];

    const int b = blockIdx.x / LEVEL_CHUNKS;
    const int chunk = blockIdx.x % LEVEL_CHUNKS;
    const int nl = __builtin_amdgcn_readfirstlane(nlev[b]);   // (scalar: loop bound)
    if (chunk >= nl) return;
    const int wpr = (W + 31) / 32;
    const int NW = H * wpr;
    const int BW = (W + 1) / 2, BH = (H + 1) / 2, NB = BH * BW;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    // psi of this thread's bitmap words -> registers (8 packed dwords/word).
    uint32_t pv[QW][8];
    const uint8_t* src = psi_g + (long)b * H * W;
#pragma unroll
    for (int q = 0; q < QW; ++q) {
        const int w = tid + q * NTB;
#pragma unroll
        for (int d = 0; d < 8; ++d) pv[q][d] = 0u;
        if (w < NW) {
            const int y = w / wpr, x0 = (w - y * wpr) * 32;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                uint32_t v = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int x = x0 + 4 * d + e;
                    if (x < W) v |= (uint32_t)src[y * W + x] << (8 * e);
                }
                pv[q][d] = v;
            }
        }
    }
    LevelCtx cx{bm, H, W, wpr, BW};

    for (int li = chunk; li < nl; li += LEVEL_CHUNKS) {
        const int L = lev_list[b * 256 + li];
        int32_t* box = boxes + ((long)b * 256 + L) * 4;
        // 1. bitmap F = {psi > L}.
#pragma unroll
        for (int q = 0; q < QW; ++q) {
            const int w = tid + q * NTB;
            if (w < NW) {
                uint32_t bits = 0;
#pragma unroll
                for (int d = 0; d < 8; ++d)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        bits |= (uint32_t)(((pv[q][d] >> (8 * e)) & 255u) > (uint32_t)L) << (4 * d + e);
                bm[w] = bits;
            }
        }
        __syncthreads();
        PHASE(0);
        // 2. horizontal runs: one wave per block row, one lane per block
        // (two passes of 64 blocks); a block starts a run unless its left
        // column touches the right column of an active left neighbour.  Each
        // active block points at its run start (trees of depth 1).
        for (int by = wid; by < BH; by += NTB / 64) {
            const int y = 2 * by;
            int carry = -1;   // run start of the last block of the previous pass
            for (int base = 0; base < BW; base += 64) {
                const int bx = base + lane;
                int t = 0, u = 0, tl = 0, ul = 0;
                if (bx < BW) {
                    t = cx.pair(y, 2 * bx);
                    u = cx.pair(y + 1, 2 * bx);
                    if (bx > 0) {
                        tl = cx.bit(y, 2 * bx - 1);
                        ul = cx.bit(y + 1, 2 * bx - 1);
                    }
                }
                const bool act = (t | u) != 0;
                const bool joined = act && ((t | u) & 1) && (tl | ul);
                const uint64_t starts = __ballot(act && !joined);
                const uint64_t acts = __ballot(act);
                // run start = highest start bit <= lane, or the carry
                const uint64_t below = lane == 63 ? starts : (starts & ((2ull << lane) - 1));
                int head = below ? base + 63 - __builtin_clzll(below) : carry;
                if (bx < BW) lab[by * BW + bx] = act ? (uint32_t)(by * BW + head) : INACT;
                // carry for the next pass: the run of block base+63 if it is active
                const int last = __shfl(head, 63, 64);
                carry = ((acts >> 63) & 1) ? last : -1;
            }
        }
        __syncthreads();
        PHASE(1);
        // 3. union with the top-left, top and top-right blocks (hooks toward
        // the smaller root with atomicMin; only run heads are ever roots).
        // Lanes take consecutive blocks (conflict-free LDS); a lane skips an
        // upper block whose run start equals the one its left neighbour lane
        // just united for the same run (wave-level dedupe of wide overlaps).
        for (int i0 = 0; i0 < NB; i0 += NTB) {
            const int i = i0 + tid;
            uint32_t hi = INACT, ht = INACT, hl = INACT, hr = INACT;
            if (i < NB && i >= BW) {
                hi = lab[i];
                if (hi != INACT) {
                    const int by = i / BW, bx = i - by * BW, y = 2 * by, x = 2 * bx;
                    const int top = cx.pair(y, x);         // bit0 = (y,x), bit1 = (y,x+1)
                    if (top) {
                        if (cx.pair(y - 1, x)) ht = lab[i - BW];
                        if (bx > 0 && (top & 1) && cx.bit(y - 1, x - 1)) hl = lab[i - BW - 1];
                        if (bx + 1 < BW && (top & 2) && cx.bit(y - 1, x + 2)) hr = lab[i - BW + 1];
                    }
                }
            }
            // left neighbour lane's (run, targets)
            const uint32_t phi = __shfl_up(hi, 1, 64);
            const uint32_t pht = __shfl_up(ht, 1, 64);
            const uint32_t phr = __shfl_up(hr, 1, 64);
            const bool same_run = lane > 0 && phi == hi && (i % BW) != 0;
            auto seen = [&](uint32_t h) { return same_run && (h == pht || h == phr); };
            if (hi != INACT) {
                if (hl != INACT && !seen(hl)) unite(lab, hi, hl);
                if (ht != INACT && !seen(ht)) unite(lab, hi, ht);
                if (hr != INACT && !seen(hr)) unite(lab, hi, hr);
            }
        }
        __syncthreads();
        PHASE(2);
        // 4. pointer jumping on run heads until every head points at its
        // root, then every block takes its head's root; 5. root slots become
        // area accumulators.
        // pointer doubling until every block points at its root (only run
        // starts were ever hooked, so chains are short).
        for (;;) {
            int ch = 0;
            for (int i = tid; i < NB; i += NTB) {
                const uint32_t v = lab[i];
                if (v == INACT || v == (uint32_t)i) continue;
                const uint32_t w = lab[v];
                if (w != v) { lab[i] = w; ch = 1; }
            }
            ch = block_max_i(ch, red);
            if (!ch) break;
        }
        for (int i = tid; i < NB; i += NTB)
            if (lab[i] == (uint32_t)i) lab[i] = RFLAG;
        __syncthreads();
        PHASE(3);
        // 6. window areas in half units: per 32-window strip, windows with
        // >= 3 pixels in F form runs; one run = one component (adjacent
        // windows share two pixels, at least one of them in F).
        {
            const int nsj = (W + 1 + 31) / 32;   // strips per window row (wx in [-1, W-1])
            const int nstrips = (H + 1) * nsj;
            const int per = (nstrips + NTB - 1) / NTB;
            uint32_t cr = INACT, cacc = 0;   // local (root, sum) cache
            for (int st = tid * per; st < min(nstrips, (tid + 1) * per); ++st) {
                const int wy = st / nsj - 1, j = st % nsj;
                // window wx = 32j - 1 + i covers pixels x = 32j - 1 + i, 32j + i
                const uint32_t t0 = cx.word(wy, j), t1 = cx.word(wy + 1, j);
                const uint32_t tp = cx.word(wy, j - 1), bp = cx.word(wy + 1, j - 1);
                const uint32_t tl = (t0 << 1) | (tp >> 31), tr = t0;
                const uint32_t bl = (t1 << 1) | (bp >> 31), br = t1;
                uint32_t m3 = (tl & tr & (bl | br)) | (bl & br & (tl | tr));
                const uint32_t m4 = tl & tr & bl & br;
                const int nvalid = W + 1 - 32 * j;          // windows in this strip
                if (nvalid < 32) m3 &= (1u << nvalid) - 1u;
                while (m3) {
                    const int s0 = __builtin_ctz(m3);
                    const uint32_t rest = ~(m3 >> s0);
                    const int len = rest ? __builtin_ctz(rest) : 32 - s0;
                    const uint32_t run = (len >= 32 ? 0xFFFFFFFFu : ((1u << len) - 1u)) << s0;
                    const uint32_t contrib = __builtin_popcount(run) + __builtin_popcount(m4 & run);
                    // an F pixel of window s0
                    const int wx = 32 * j - 1 + s0;
                    int py, px;
                    if ((tl >> s0) & 1) { py = wy; px = wx; }
                    else if ((tr >> s0) & 1) { py = wy; px = wx + 1; }
                    else if ((bl >> s0) & 1) { py = wy + 1; px = wx; }
                    else { py = wy + 1; px = wx + 1; }
                    const uint32_t r = root_of(lab, (py >> 1) * BW + (px >> 1));
                    if (r != cr) {
                        if (cr != INACT) atomicAdd(&lab[cr], cacc);
                        cr = r;
                        cacc = 0;
                    }
                    cacc += contrib;
                    m3 &= ~run;
                }
            }
            if (cr != INACT) atomicAdd(&lab[cr], cacc);
        }
        __syncthreads();
        PHASE(4);
        // 7. max area over roots.
        int ma = -1;
        for (int i = tid; i < NB; i += NTB) {
            const uint32_t v = lab[i];
            if (v != INACT && (v & RFLAG)) ma = max(ma, (int)(v & ~RFLAG));
        }
        ma = block_max_i(ma, red);
        // 8. candidates (area == max) get a key slot; others NOKEY.
        for (int i = tid; i < NB; i += NTB) {
            const uint32_t v = lab[i];
            if (v != INACT && (v & RFLAG))
                lab[i] = ((int)(v & ~RFLAG) == ma) ? (RFLAG | 0x7FFFFFFEu) : NOKEY;
        }
        __syncthreads();
        // 9. key = 1 + raster index of the component's first pixel.
        // The root is the component's smallest block index, so its first
        // pixel lies in the root's block row: only those blocks compete.
        for (int i = tid; i < NB; i += NTB) {
            if (lab[i] == INACT) continue;
            const uint32_t r = root_of(lab, i);
            const int by = i / BW;
            if ((int)r / BW != by || lab[r] == NOKEY) continue;
            const int x = 2 * (i - by * BW), y = 2 * by;
            const int top = cx.pair(y, x);
            int k;
            if (top & 1) k = y * W + x;
            else if (top & 2) k = y * W + x + 1;
            else if (cx.bit(y + 1, x)) k = (y + 1) * W + x;
            else k = (y + 1) * W + x + 1;
            atomicMin(&lab[r], RFLAG | (uint32_t)(k + 1));
        }
        __syncthreads();
        // 10. winner = candidate with the largest key (first in OpenCV's list).
        int best = 0;
        for (int i = tid; i < NB; i += NTB) {
            const uint32_t v = lab[i];
            if (v != INACT && (v & RFLAG) && v != NOKEY) best = max(best, (int)(v & ~RFLAG));
        }
        best = block_max_i(best, red);
        const int fp = best - 1;
        const uint32_t wroot = root_of(lab, ((fp / W) >> 1) * BW + ((fp % W) >> 1));
        PHASE(5);
        // 11. bbox of the winner (4 reductions in one pass).
        int x0 = W, y0 = H, x1 = -1, y1 = -1;
        for (int i = tid; i < NB; i += NTB) {
            if (lab[i] == INACT || root_of(lab, i) != wroot) continue;
            const int by = i / BW, x = 2 * (i - by * BW), y = 2 * by;
            const int top = cx.pair(y, x), bot = cx.pair(y + 1, x);
            if (top | bot) {
                x0 = min(x0, ((top | bot) & 1) ? x : x + 1);
                x1 = max(x1, ((top | bot) & 2) ? x + 1 : x);
                y0 = min(y0, top ? y : y + 1);
                y1 = max(y1, bot ? y + 1 : y);
            }
        }
        x0 = wave_min_i(x0); y0 = wave_min_i(y0);
        x1 = wave_max_i(x1); y1 = wave_max_i(y1);
        if (lane == 0) {
            red[4 * wid + 0] = x0; red[4 * wid + 1] = y0;
            red[4 * wid + 2] = x1; red[4 * wid + 3] = y1;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NTB / 64; ++w) {
                x0 = min(x0, red[4 * w + 0]); y0 = min(y0, red[4 * w + 1]);
                x1 = max(x1, red[4 * w + 2]); y1 = max(y1, red[4 * w + 3]);
            }
            box[0] = x0;
            box[1] = y0;
            box[2] = min(x1 + 1, W - 1);  // boundingRect x + w, clamped (wsol_metrics.py:175-178)
            box[3] = min(y1 + 1, H - 1);
        }
        __syncthreads();
        PHASE(6);
    }
    if (dbg && tid == 0) {
        uint64_t* d = dbg + (long)(gridDim.x + blockIdx.x) * DBG_SLOTS;
        for (int k = 0; k < 7; ++k) d[k] = ph[k];
    }
}

// Fill the rows of non-canonical levels from their canonical level.
__global__ void expand_kernel(const int32_t* __restrict__ canon, const int32_t* __restrict__ vmax,
                              int32_t* __restrict__ boxes, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 256) return;
    const int b = i / 256, L = i % 256;
    if (L >= vmax[b]) return;
    const int c = canon[b * 256 + L];
    if (c == L) return;
    const int32_t* s = boxes + ((long)b * 256 + c) * 4;
    int32_t* d = boxes + ((long)b * 256 + L) * 4;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
}

// ------------------------------------------------------------ accumulate
__global__ void accumulate_kernel(const int32_t* __restrict__ boxes,
                                  const int32_t* __restrict__ vmax, const double* __restrict__ taus,
                                  int T, const int32_t* __restrict__ gt,
                                  const int32_t* __restrict__ ngt, int G,
                                  const int32_t* __restrict__ top1,
                                  const int32_t* __restrict__ top5,
                                  const double* __restrict__ iou_thr, int n_iou,
                                  int32_t* __restrict__ counters, double* __restrict__ best_iou,
                                  int B) {
    long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)B * T) return;
    const int b = (int)(id / T), i = (int)(id % T);
    const int vm = vmax[b];
    // thresh = int(threshold * np.max(scoremap_image))  (wsol_metrics.py:158)
    const int thr = (int)(taus[i] * (double)vm);
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    if (thr < vm) {
        const int32_t* bx = boxes + ((long)b * 256 + thr) * 4;
        a0 = bx[0]; a1 = bx[1]; a2 = bx[2]; a3 = bx[3];
    }
    // calculate_multiple_iou (wsol_metrics.py:77-124), max over GT boxes.
    double best = 0.0;
    const int ng = ngt[b];
    for (int g = 0; g < ng; ++g) {
        const int32_t* q = gt + ((long)b * G + g) * 4;
        long mnx = max(a0, q[0]), mny = max(a1, q[1]);
        long mxx = min(a2, q[2]), mxy = min(a3, q[3]);
        long inter = max(0L, mxx - mnx + 1) * max(0L, mxy - mny + 1);
        long area_a = (long)(a2 - a0 + 1) * (a3 - a1 + 1);
        long area_b = (long)(q[2] - q[0] + 1) * (q[3] - q[1] + 1);
        long den = area_a + area_b - inter;
        double iou = den <= 0 ? 0.0 : (double)inter / (double)den;
        if (g == 0 || iou > best) best = iou;
    }
    if (best_iou) best_iou[id] = best;
    for (int j = 0; j < n_iou; ++j) {
        if (best >= iou_thr[j]) {
            atomicAdd(&counters[(0 * n_iou + j) * T + i], 1);
            if (top1[b]) atomicAdd(&counters[(1 * n_iou + j) * T + i], 1);
            if (top5[b]) atomicAdd(&counters[(2 * n_iou + j) * T + i], 1);
        }
    }
}

// ---- sorted-list level sweep (frames <= 224 x 224, default).  The level sets F_L = {psi > L}
// are nested: going down the listed levels only ADDS pixels, so components only grow and
// merge.  A workgroup takes a contiguous range of one frame's levels (INC_CHUNKS ranges per
// frame) and walks it from the top; the pixels new at a level are a slice of the frame's pixel
// list sorted by psi (the fill writes it, emit_sorted), so no level thresholds psi or compacts
// a list — the slice sets its bits in the level bitmaps and stages itself in LDS (the range's
// first level takes every pixel above it).  Kept across levels:
//  * per 2x2 block (all its set pixels are 8-adjacent, so block labels are pixel labels) the
//    union-find parent, hooked toward the smaller block index: a root is its component's first
//    block in raster order;
//  * per root the raster index of its component's first pixel, the key.  Parent and key share
//    one word (pk = parent << 16 | key; key 0xFFFF on non-roots and on roots that hold no pixel
//    yet; INACT = block not active), so the hook that makes a root a child, an atomicMin with
//    key 0xFFFF, also clears its key and returns it for the handover;
//  * per root the window area in half units (the shoelace area of the header comment).  Window
//    areas are additive over components because all set pixels of a 2x2 window are 8-adjacent
//    (one component): every window that holds a new pixel adds contrib(new count) -
//    contrib(old count), once, by its first new pixel in raster order;
//  * per root its component's bounding box (x0, x1 in xr, y1 in the top byte of its area word,
//    y0 = key / W), widened by its new pixels and merged on a hook, so the winner's box is read
//    off its root: no pass over the blocks, whatever merged.
// Per level only the new pixels are visited: their blocks become active, they unite with the
// blocks of their set 8-neighbours, and the roots hooked this level — unite_pk lists them, so
// no step scans all blocks to find them — pass their area, key and box on to their new root.
// The winner is max(area, then key) — the same as level_kernel (largest area, ties to the last
// first-pixel in raster order = the first contour in OpenCV's list) — taken over the roots
// TOUCHED this level only (roots of the new pixels, roots that took a hooked root in, the
// previous winner's root): every other root kept its value, which was below the previous
// winner's.  Only when the new maximum is below the previous winner's value (its key fell with
// no area gain) does a full pass over the roots decide.
// Paths are compressed only where the winner search walks them (the touched blocks); a
// compression pass over all blocks on the merge levels measured slower than the longer paths it
// saves (TCAM_BBOX_COMPRESS=1).
// Bit-identical to level_kernel (tests/test_gpu_ops.py).
// One range per frame (the whole level list in one workgroup) by default: a workgroup holds
// a CU's whole LDS, so the side stream's cost to the pipelined forward is its CU-time, and a
// second range per frame re-does the levels above it (profiles/round3_bbox_chunks.txt: the
// bbox stage's cost to the pipelined bench 6.7 -> 4.8 %, at 2x the per-clip latency, which the
// next clip's forward hides).
constexpr int INC_CHUNKS = 1;      // default level ranges per frame
constexpr int INC_MAX_CHUNKS = 4;  // workspace is sized for this many
constexpr int IH = 224, IW = 224, IWPR = 7, IBW = 112, INB = IBW * (IH / 2);
constexpr int SCAP = INB;                          // new-pixel entries staged in LDS
constexpr uint32_t SAMASK = (1u << 17) - 1;        // ar word: area (half units) | y1 << 24
constexpr uint32_t XR_EMPTY = 0x00FFu;             // xr half-word: x0 | x1 << 8; empty box

// parent-key words: parent in the high half
__device__ inline uint32_t find_root_pk(const uint32_t* pk, uint32_t x) {
    uint32_t p = pk[x] >> 16;
    while (p != x) {
        x = p;
        p = pk[x] >> 16;
    }
    return x;
}

// unite() on parent-key words: the hook of root b under a is atomicMin(pk[b], a << 16 |
// 0xFFFF) — it also clears b's key, which the returned old word still holds; every hooked
// root is appended to hl as (b << 16 | key).  (A block is hooked at most once: afterwards it
// is no longer a root.)
__device__ inline void unite_pk(uint32_t* pk, uint32_t a, uint32_t b, uint32_t* hl, int* nh) {
    for (;;) {
        a = find_root_pk(pk, a);
        b = find_root_pk(pk, b);
        if (a == b) return;
        if (a > b) { uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&pk[b], a << 16 | 0xFFFFu);
        if ((old >> 16) == b) {
            hl[atomicAdd(nh, 1)] = b << 16 | (old & 0xFFFFu);
            return;
        }
        b = old >> 16;
    }
}

__device__ inline int win_contrib(int c) { return c == 4 ? 2 : (c == 3 ? 1 : 0); }

__device__ inline uint32_t lds_ld(const uint32_t* p) { return *(const volatile uint32_t*)p; }

// y1 field (bits 24..31) of an area word <- max(y1, y); the area bits may change under
// concurrent atomicAdds, hence the CAS loop
__device__ inline void ar_max_y1(uint32_t* w, uint32_t y) {
    uint32_t old = lds_ld(w);
    while ((old >> 24) < y) {
        const uint32_t prev = atomicCAS(w, old, (old & 0x00FFFFFFu) | (y << 24));
        if (prev == old) return;
        old = prev;
    }
}

// x-range half-word of root r (two per word) <- [min(x0, .), max(x1, .)]
__device__ inline void xr_widen(uint32_t* xr, uint32_t r, uint32_t x0, uint32_t x1) {
    uint32_t* w = xr + (r >> 1);
    const int sh = (int)(r & 1u) * 16;
    uint32_t old = lds_ld(w);
    for (;;) {
        const uint32_t cur = (old >> sh) & 0xFFFFu;
        const uint32_t nv = min(cur & 255u, x0) | max(cur >> 8, x1) << 8;
        if (nv == cur) return;
        const uint32_t prev = atomicCAS(w, old, (old & ~(0xFFFFu << sh)) | (nv << sh));
        if (prev == old) return;
        old = prev;
    }
}

// block-wide max without the serial combine: every thread reads the 16 wave maxima
__device__ inline unsigned long long block_max_u64_all(unsigned long long v,
                                                       unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NTB / 64; ++i) v = red[i] > v ? red[i] : v;
    return v;
}

__global__ __launch_bounds__(NTB) void level_sorted_kernel(
    const uint16_t* __restrict__ slist_g, const int32_t* __restrict__ cgt_g,
    const int32_t* __restrict__ lev_list, const int32_t* __restrict__ nlev,
    int32_t* __restrict__ boxes, int H, int W, uint32_t* __restrict__ hlist_g,
    uint64_t* __restrict__ dbg, int nch, int compress) {
    uint64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t n_comp = 0, n_fallback = 0;   // (debug) compression passes, full winner passes
    uint64_t tp = rt();
    __shared__ uint32_t bm[IH * IWPR];    // F at the current level
    __shared__ uint32_t db[IH * IWPR];    // pixels new at the current level
    __shared__ uint32_t pk[INB];          // parent << 16 | key
    __shared__ uint32_t ar[INB];          // per root: area (half units) | y1 << 24
    __shared__ uint32_t xr[INB / 2];      // per root: x0 | x1 << 8 (uint16 pairs)
    __shared__ uint16_t lst[SCAP];        // this level's new pixels, if they fit
    __shared__ unsigned long long redl[NTB / 64 + 1];
    __shared__ int s_nhook, s_nmerge;
    __shared__ unsigned long long s_pbest, s_best;
    const int b = blockIdx.x / nch, chunk = blockIdx.x % nch;
    uint32_t* hlist = hlist_g + (long)blockIdx.x * INB;
    const uint16_t* slist = slist_g + (long)b * H * W;
    const int32_t* cgt = cgt_g + (long)b * 257;
    // (block-uniform values that steer loops and branches holding barriers or cross-lane
    // ops are read into scalars, so the compiler cannot treat those as divergent)
    const int nl = __builtin_amdgcn_readfirstlane(nlev[b]);
    const int l0 = nl * chunk / nch, l1 = nl * (chunk + 1) / nch;
    if (l0 >= l1) return;
    const int wpr = (W + 31) / 32, NW = H * wpr;
    const int BW = (W + 1) / 2, BH = (H + 1) / 2, NB = BH * BW;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int i = tid; i < NB; i += NTB) {
        pk[i] = INACT;
        ar[i] = 0;
    }
    for (int i = tid; i < (NB + 1) / 2; i += NTB) xr[i] = XR_EMPTY | XR_EMPTY << 16;
    for (int w = tid; w < NW; w += NTB) bm[w] = 0u;
    if (tid == 0) s_pbest = 0;
    LevelCtx cx{bm, H, W, wpr, BW};
    uint32_t pwin = INACT;                 // previous level's winner root
    auto isnew = [&](int y, int x) -> int {
        if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0;
        return (db[y * wpr + (x >> 5)] >> (x & 31)) & 1;
    };
    int s_hi = 0;   // list entries [0, s_hi) are set

    for (int li = l1 - 1; li >= l0; --li) {
        const int L = __builtin_amdgcn_readfirstlane(lev_list[b * 256 + li]);
        // (the range's first level takes everything above; clamped so that inconsistent
        // level tables cannot send a read outside the frame's list)
        const int s0 = s_hi, s1 = min(max(__builtin_amdgcn_readfirstlane(cgt[L]), s0), H * W);
        s_hi = s1;
        const int nnew = s1 - s0;
        const bool inl = nnew <= SCAP;      // (block-uniform) the slice is staged in LDS
        for (int w = tid; w < NW; w += NTB) db[w] = 0u;
        if (tid == 0) {
            s_nhook = 0;
            s_nmerge = 0;
            s_best = 0;
        }
        __syncthreads();
        PHASE(0);
        // 1. the slice: bits of F and of the new set, LDS copy, blocks become active (roots
        // of themselves; a block, once active, stays active)
        for (int it = tid; it < nnew; it += NTB) {
            const uint32_t pp = slist[s0 + it];
            if (inl) lst[it] = (uint16_t)pp;
            const int y = (int)(pp >> 8), x = (int)(pp & 255);
            const uint32_t bit = 1u << (x & 31);
            atomicOr(&bm[y * wpr + (x >> 5)], bit);
            atomicOr(&db[y * wpr + (x >> 5)], bit);
            const uint32_t blk = (y >> 1) * BW + (x >> 1);
            if (pk[blk] == INACT) pk[blk] = blk << 16 | 0xFFFFu;
        }
        __syncthreads();
        auto newpx = [&](int it) -> uint32_t { return inl ? (uint32_t)lst[it] : slist[s0 + it]; };
        PHASE(1);
        // 2. new pixels unite their block with the adjacent blocks that hold a set 8-neighbour:
        // a pixel's 8 neighbours outside its own block lie in three blocks — horizontal
        // (2 pixels), vertical (2) and diagonal (1) — one lane per (pixel, block)
        for (int it = tid; it < nnew * 3; it += NTB) {
            const int q = it / 3, k = it - 3 * q;
            const uint32_t pp = newpx(q);
            const int y = (int)(pp >> 8), x = (int)(pp & 255);
            const int sy = (y & 1) ? 1 : -1, sx = (x & 1) ? 1 : -1;   // toward the outside
            int ny, nx, set;
            if (k == 0) {        // horizontal block
                ny = y; nx = x + sx;
                set = cx.bit(y, nx) | cx.bit(y - sy, nx);
            } else if (k == 1) { // vertical block
                ny = y + sy; nx = x;
                set = cx.bit(ny, x) | cx.bit(ny, x - sx);
            } else {             // diagonal block
                ny = y + sy; nx = x + sx;
                set = cx.bit(ny, nx);
            }
            if (set)
                unite_pk(pk, (y >> 1) * BW + (x >> 1), (ny >> 1) * BW + (nx >> 1), hlist,
                         &s_nhook);
        }
        __syncthreads();
        PHASE(2);
        // 3. roots hooked this level that held pixels hand their area, key and box to their
        // new root (roots activated this level hold none yet: key 0xFFFF)
        const int nhook = s_nhook;
        const volatile uint32_t* hlv = hlist;
        for (int it = tid; it < nhook; it += NTB) {
            const uint32_t e = hlv[it], i = e >> 16, k = e & 0xFFFFu;
            if (k != 0xFFFFu) {
                const uint32_t r = find_root_pk(pk, i);
                const uint32_t a = ar[i];
                const uint32_t xi = (xr[i >> 1] >> ((i & 1u) * 16)) & 0xFFFFu;
                atomicAdd(&ar[r], a & SAMASK);
                ar_max_y1(&ar[r], a >> 24);
                xr_widen(xr, r, xi & 255u, xi >> 8);
                atomicMin(&pk[r], r << 16 | k);
                s_nmerge = 1;   // benign same-value race
            }
        }
        // (no barrier: step 4 only updates current roots, which step 3 never reads from,
        // and the updates commute)
        PHASE(3);
        // 4. window-area deltas (one lane per (pixel, window)), first-pixel keys, and the
        // box of each root widened by its new pixels
        for (int it = tid; it < nnew * 4; it += NTB) {
            {
                const uint32_t pp = newpx(it >> 2);
                const int y = (int)(pp >> 8), x = (int)(pp & 255);
                const uint32_t r = find_root_pk(pk, (y >> 1) * BW + (x >> 1));
                if ((it & 3) == 0) atomicMin(&pk[r], r << 16 | (uint32_t)(y * W + x));
                const int wy = y - 1 + ((it >> 1) & 1), wx = x - 1 + (it & 1);
                int cn = 0, co = 0;
                bool owner = true;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int qy = wy + (k >> 1), qx = wx + (k & 1);
                    const int nbit = cx.bit(qy, qx), nw = isnew(qy, qx);
                    cn += nbit;
                    co += nbit & (nw ^ 1);
                    // an earlier (raster order) new pixel of this window owns it
                    if (nw && (qy < y || (qy == y && qx < x))) owner = false;
                }
                const int dsum = owner ? win_contrib(cn) - win_contrib(co) : 0;
                if (dsum) atomicAdd(&ar[r], (uint32_t)dsum);
                // (both read first and write only a pixel that lies outside the box)
                if ((it & 3) == 0) {
                    xr_widen(xr, r, (uint32_t)x, (uint32_t)x);
                    ar_max_y1(&ar[r], (uint32_t)y);
                }
            }
        }
        __syncthreads();
        PHASE(4);
        // 5. path compression after merges; the winner over the touched roots (each touched
        // block's path compressed on the way: no unites run in this step, and a non-root
        // re-pointed at its root keeps every find_root correct)
        if (__builtin_amdgcn_readfirstlane(s_nmerge) && compress) {
            ++n_comp;
            for (int i = tid; i < NB; i += NTB) {
                const uint32_t w = pk[i];
                if (w == INACT || (w >> 16) == (uint32_t)i) continue;
                const uint32_t p = w >> 16;
                if ((pk[p] >> 16) == p) continue;
                pk[i] = find_root_pk(pk, p) << 16 | 0xFFFFu;
            }
        }
        unsigned long long best = 0;
        auto cand = [&](uint32_t x) {
            const uint32_t r = find_root_pk(pk, x);
            if (r != x) pk[x] = r << 16 | 0xFFFFu;
            const unsigned long long a =
                ((unsigned long long)(ar[r] & SAMASK) << 32) | (pk[r] & 0xFFFFu);
            best = a > best ? a : best;
        };
        for (int it = tid; it < nnew; it += NTB) {
            const uint32_t pp = newpx(it);
            cand(((pp >> 8) >> 1) * BW + ((pp & 255) >> 1));
        }
        for (int it = tid; it < nhook; it += NTB) cand(hlv[it] >> 16);
        if (tid == 0 && pwin != INACT) cand(pwin);
        PHASE(5);
        // block max: wave max, one LDS atomicMax per wave, one barrier
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(best, o, 64);
            best = t > best ? t : best;
        }
        if (lane == 0 && best) atomicMax(&s_best, best);
        __syncthreads();
        best = s_best;
        if (__builtin_amdgcn_readfirstlane((int)(best < s_pbest))) {
            ++n_fallback;
            // the previous winner's value fell (its key dropped with no area gain): an
            // untouched root may now lead, so every root decides
            best = 0;
            for (int i = tid; i < NB; i += NTB) {
                const uint32_t v = pk[i];
                if ((v >> 16) == (uint32_t)i) {
                    const unsigned long long a =
                        ((unsigned long long)(ar[i] & SAMASK) << 32) | (v & 0xFFFFu);
                    best = a > best ? a : best;
                }
            }
            best = block_max_u64_all(best, redl);
        }
        const uint32_t fp = (uint32_t)best;   // the winner's first pixel
        const uint32_t wroot = find_root_pk(pk, ((fp / W) >> 1) * BW + ((fp % W) >> 1));
        PHASE(6);
        // 6. its box, off the root
        if (tid == 0) {
            const uint32_t xw = (xr[wroot >> 1] >> ((wroot & 1u) * 16)) & 0xFFFFu;
            int32_t* box = boxes + ((long)b * 256 + L) * 4;
            box[0] = (int)(xw & 255u);
            box[1] = (int)(fp / W);
            box[2] = min((int)(xw >> 8) + 1, W - 1);   // boundingRect x + w, clamped
            box[3] = min((int)(ar[wroot] >> 24) + 1, H - 1);   // (wsol_metrics.py:175-178)
            s_pbest = best;
        }
        pwin = wroot;
        __syncthreads();
        PHASE(7);
    }
    if (dbg && tid == 0) {
        uint64_t* d = dbg + (long)blockIdx.x * DBG_SLOTS;
        for (int k = 0; k < 8; ++k) d[k] = ph[k];
        d[8] = l1 - l0;
        d[9] = n_comp;
        d[10] = n_fallback;
    }
#undef PHASE
}
}  // namespace

// Workspace layout (tcam_bbox_ws_bytes):
//   psi (B x H x W uint8), padded to 16 bytes
//   | canon (B x 256 int32) | lev_list (B x 256 int32) | nlev (B int32), padded to 256 bytes
//   | hooked-root lists of the sorted sweep (B * INC_MAX_CHUNKS x 112^2 uint32: one per
//     workgroup; a block is hooked at most once)
//   | psi-sorted pixel lists (B x H x W uint16), padded to 256 bytes
//   | their level offsets, cgt (B x 257 int32)
static size_t tables_offset(int B, int H, int W) {
    return ((size_t)B * H * W + 15) / 16 * 16;
}

static size_t hook_list_offset(int B, int H, int W) {
    return (tables_offset(B, H, W) + (size_t)B * (256 + 256 + 1) * sizeof(int32_t) + 255) / 256 *
           256;
}

static size_t sorted_list_offset(int B, int H, int W) {
    return hook_list_offset(B, H, W) + (size_t)B * INC_MAX_CHUNKS * INB * sizeof(uint32_t);
}

static size_t sorted_cgt_offset(int B, int H, int W) {
    return (sorted_list_offset(B, H, W) + (size_t)B * H * W * sizeof(uint16_t) + 255) / 256 * 256;
}

extern "C" void tcam_bbox_set_chunks(int n) { g_bbox_chunks = n; }

extern "C" size_t tcam_bbox_ws_bytes(int B, int H, int W) {
    return sorted_cgt_offset(B, H, W) + (size_t)B * 257 * sizeof(int32_t);
}

extern "C" int tcam_bbox_levels(const uint8_t* cam_u8, int32_t* boxes, int32_t* vmax,
                                void* ws, int B, int H, int W, void* stream) {
    TCAM_REQUIRE(cam_u8 && boxes && vmax && ws && B > 0);
    TCAM_REQUIRE(H > 0 && W > 0 && H <= BIGH && W <= BIGW);
    hipStream_t st = as_stream(stream);
    char* base = (char*)ws;
    uint8_t* psi = (uint8_t*)ws;
    int32_t* canon = (int32_t*)(base + tables_offset(B, H, W));
    int32_t* lev_list = canon + (size_t)B * 256;
    int32_t* nlev = lev_list + (size_t)B * 256;
    uint32_t* hooks = (uint32_t*)(base + hook_list_offset(B, H, W));
    // the frame sizes that the kernels serve (the table in the header comment)
    const bool upto224 = H <= IH && W <= IW, upto256 = H <= MAXH && W <= MAXW;
    // the sorted sweep takes the level stage up to 224^2, unless level_kernel is asked for
    // as the cross-check or for its phase times (tcam_bbox_set_debug)
    const bool sorted = upto224 && g_level_variant == 0 && !g_dbg;
    // it alone reads the psi-sorted pixel list, which the fill writes when given one
    uint16_t* slist = sorted ? (uint16_t*)(base + sorted_list_offset(B, H, W)) : nullptr;
    int32_t* cgt = sorted ? (int32_t*)(base + sorted_cgt_offset(B, H, W)) : nullptr;

    // ---- fill
    if (!upto256)                  // up to 320^2: psi alone in LDS
        fill_kernel<BIGH, BIGP, false><<<B, NTB, 0, st>>>(cam_u8, psi, vmax, canon, lev_list,
                                                          nlev, H, W, g_dbg, slist, cgt);
    else if (g_fill_variant == 1)  // the cross-check, up to 256^2
        fill_kernel<MAXH, MAXP, true><<<B, NTB, 0, st>>>(cam_u8, psi, vmax, canon, lev_list,
                                                         nlev, H, W, g_dbg, slist, cgt);
    else                           // up to 256^2
        fill_scan_kernel<<<B, NTS, 0, st>>>(cam_u8, psi, vmax, canon, lev_list, nlev, H, W, slist,
                                            cgt, g_dbg, g_fill_waves, g_fill_maxit);
    TCAM_CHECK_LAUNCH();

    // ---- level stage
    // debug layout: fill rows [0, B*16) x DBG_SLOTS, level rows follow
    // level ranges per frame: more ranges = shorter latency, more CU-time (each range
    // rebuilds its top level from scratch); TCAM_BBOX_INC_CHUNKS (1..4) for A/B runs
    static const int nch = [] {
        const char* e = getenv("TCAM_BBOX_INC_CHUNKS");
        const int v = e ? atoi(e) : INC_CHUNKS;
        return v >= 1 && v <= INC_MAX_CHUNKS ? v : INC_CHUNKS;
    }();
    // (round 5) a per-call override (tcam_bbox_set_chunks): the evaluator's last clip, whose
    // sweep nothing else overlaps, runs on more ranges per frame for a shorter drain
    const int nc = (g_bbox_chunks >= 1 && g_bbox_chunks <= INC_MAX_CHUNKS) ? g_bbox_chunks : nch;
    // a compression pass over the blocks on merge levels: off by default (TCAM_BBOX_COMPRESS=1
    // for A/B runs: 1.94 vs 1.83 ms per 32-frame clip — the unites' longer paths cost less
    // than the passes)
    static const int compress = [] {
        const char* e = getenv("TCAM_BBOX_COMPRESS");
        return e ? atoi(e) : 0;
    }();
    if (sorted)        // up to 224^2
        level_sorted_kernel<<<B * nc, NTB, 0, st>>>(slist, cgt, lev_list, nlev, boxes, H, W, hooks,
                                                    g_inc_dbg, nc, compress);
    else if (upto256)  // up to 256^2, and the cross-check below that
        level_kernel<MAXH, MAXW, 2><<<B * LEVEL_CHUNKS, NTB, 0, st>>>(psi, vmax, lev_list, nlev,
                                                                      boxes, H, W, g_dbg);
    else               // up to 320^2
        level_kernel<BIGH, BIGW, 4><<<B * LEVEL_CHUNKS, NTB, 0, st>>>(psi, vmax, lev_list, nlev,
                                                                      boxes, H, W, g_dbg);
    TCAM_CHECK_LAUNCH();
    expand_kernel<<<cdiv((long)B * 256, 256), 256, 0, st>>>(canon, vmax, boxes, B);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

// Test hook: one line sweep of the clamp-scan fill (mode 0: forward + backward, 1: forward)
extern "C" int tcam_bbox_scan_line(const uint8_t* p, const uint8_t* u, uint8_t* out, int n,
                                   int mode, void* stream) {
    TCAM_REQUIRE(p && u && out && n > 0 && n <= 256);
    scan_line_kernel<<<1, 64, 0, as_stream(stream)>>>(p, u, out, n, mode);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}

// Profiling hook of the sorted-list sweep: when non-null, workgroup wg of level_sorted_kernel
// writes its per-phase ticks (s_memrealtime, 100 MHz) to buf[wg*16 + 0..7], the levels it
// processed to slot 8, its compression passes to slot 9 and its full winner passes to slot 10.
// buf must hold B * chunks * 16 uint64.
extern "C" int tcam_bbox_set_inc_debug(uint64_t* buf) {
    g_inc_dbg = buf;
    return TCAM_OK;
}

// 0 = the sorted-list sweep where it applies (frames <= 224^2, default), 1 = level_kernel
// (per-level CCL, the reference check) always
extern "C" int tcam_bbox_level_variant(int v) {
    TCAM_REQUIRE(v == 0 || v == 1);
    g_level_variant = v;
    return TCAM_OK;
}

// 0 = the clamp-scan fill (default), 1 = fill_kernel (LDS sweeps, the reference check)
extern "C" int tcam_bbox_fill_variant(int v) {
    if (v >= 1000) {  // (debug) 1000 + k: at most k row + column passes (0: no limit)
        g_fill_maxit = v == 1000 ? 1 << 30 : v - 1000;
        return TCAM_OK;
    }
    if (v >= 100) {   // (debug) 100 + n: n waves sweep the lines of the clamp-scan fill
        g_fill_waves = v - 100;
        return TCAM_OK;
    }
    TCAM_REQUIRE(v == 0 || v == 1);
    g_fill_variant = v;
    return TCAM_OK;
}

// Debug/profiling hook: when non-null, the fill kernel writes per-frame phase
// times (s_memrealtime ticks, 100 MHz) to buf[b*16 + 0..4] (load, sweeps,
// histogram, iterations, and the distinct levels from fill_kernel or the
// sorted-list ticks from fill_scan_kernel) and level_kernel, which then takes
// the level stage at every frame size, accumulates per-phase ticks to
// buf[(gridDim + wg)*16 + 0..6].  buf must hold 2 * B * 16 * 16 uint64.
extern "C" int tcam_bbox_set_debug(uint64_t* buf) {
    g_dbg = buf;
    return TCAM_OK;
}

extern "C" int tcam_box_accumulate(const int32_t* boxes, const int32_t* vmax, const double* taus,
                                   int T, const int32_t* gt, const int32_t* ngt, int G,
                                   const int32_t* top1, const int32_t* top5,
                                   const double* iou_thr, int n_iou, int32_t* counters,
                                   double* best_iou, int B, void* stream) {
    TCAM_REQUIRE(boxes && vmax && taus && gt && ngt && top1 && top5 && iou_thr && counters);
    TCAM_REQUIRE(T > 0 && G > 0 && n_iou > 0 && B > 0);
    long total = (long)B * T;
    accumulate_kernel<<<cdiv(total, 256), 256, 0, as_stream(stream)>>>(
        boxes, vmax, taus, T, gt, ngt, G, top1, top5, iou_thr, n_iou, counters, best_iou, B);
    TCAM_CHECK_LAUNCH();
    return TCAM_OK;
}
