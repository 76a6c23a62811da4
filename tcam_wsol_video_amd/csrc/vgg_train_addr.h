// Index arithmetic of the VGG16 stage-1 kernels (vgg_train.hip), as host + device inline
// functions: the kernels take every byte offset from here, and tests/host/vgg_addr_check.cpp
// walks the same functions over each kernel's whole launch grid on the CPU and asserts
// offset + access bytes <= buffer bytes for every access of every thread.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VT_HD __host__ __device__ inline
#else
#define VT_HD inline
#endif

namespace vt {

constexpr int kBlock = 256;       // threads per block of every kernel here
constexpr int kMaxBlocks = 1024;  // the ReLU backward's fixed grid bound (its partial sums)

// Byte offset of 8-channel group g of pixel p in a (P pixels, G groups) tensor whose groups
// are gb bytes: 16 (S1: [h x8] fp16), 32 (S2: [h x8][l x8] fp16), 48 (S3: three bf16 parts).
VT_HD long group_off(long p, int G, int g, int gb) { return (p * G + g) * (long)gb; }

// ------------------------------------------------------------ ReLU backward + bias gradient
// A block is `per` = kBlock / G rows of G threads: thread (r, g) walks the pixels
// block * per + r, + blocks * per, ... of channel group g (consecutive groups of one pixel
// side by side: coalesced), so each channel's sum has a fixed order.
struct ReluGeom {
    long P;      // pixels
    int G;       // channel groups (C / 8), 1 .. kBlock
    int per;     // pixel rows per block
    int blocks;  // grid size
};

VT_HD bool relu_geom(long P, int C, ReluGeom* q) {
    if (P <= 0 || C <= 0 || C % 8 != 0 || C / 8 > kBlock) return false;
    q->P = P;
    q->G = C / 8;
    q->per = kBlock / q->G;
    const long nb = (P + q->per - 1) / q->per;
    q->blocks = (int)(nb < kMaxBlocks ? nb : kMaxBlocks);
    return true;
}

struct ReluThread {
    int g, r;   // channel group, pixel row within the block
    long p0;    // first pixel (-1: an idle thread, tid >= per * G)
    long step;  // pixel stride
};

VT_HD ReluThread relu_thread(const ReluGeom& q, int block, int tid) {
    ReluThread t;
    t.g = tid % q.G;
    t.r = tid / q.G;
    t.step = (long)q.blocks * q.per;
    t.p0 = t.r < q.per ? (long)block * q.per + t.r : -1;
    return t;
}

// LDS slot (of kBlock * 8) holding row r's value of channel c: thread r * G + c / 8, lane c % 8.
VT_HD int relu_lds_slot(const ReluGeom& q, int r, int c) {
    return (r * q.G + c / 8) * 8 + c % 8;
}

// The per-block partial sums: (blocks, C) doubles.
VT_HD long relu_part_off(const ReluGeom& q, int block, int c) {
    return ((long)block * q.G * 8 + c) * (long)sizeof(double);
}
VT_HD size_t relu_ws_bytes(const ReluGeom& q) {
    return (size_t)q.blocks * q.G * 8 * sizeof(double);
}

// ------------------------------------------------------------ MaxPool2d(2, 2) backward
// One thread per (frame, 2x2 window, channel group) over the ceil(H / 2) x ceil(W / 2) windows
// that tile the input: the floor(H / 2) x floor(W / 2) full ones are the pool's outputs, the
// partial ones along a last odd row / column only receive zeros.
struct PoolGeom {
    int B, G, H, W, Ho, Wo, Hc, Wc;
    long total;  // threads
};

VT_HD bool pool_geom(int B, int C, int H, int W, int Ho, int Wo, PoolGeom* q) {
    if (B <= 0 || C <= 0 || C % 8 != 0 || H < 2 || W < 2) return false;
    if (Ho != H / 2 || Wo != W / 2) return false;
    q->B = B;
    q->G = C / 8;
    q->H = H;
    q->W = W;
    q->Ho = Ho;
    q->Wo = Wo;
    q->Hc = (H + 1) / 2;
    q->Wc = (W + 1) / 2;
    q->total = (long)B * q->Hc * q->Wc * q->G;
    return true;
}

struct PoolThread {
    int g;
    long in_pix[4];  // input pixel of tap (kh, kw) = (k / 2, k % 2); -1 outside the frame
    long out_pix;    // the window's output pixel; -1 for a partial window
};

VT_HD PoolThread pool_thread(const PoolGeom& q, long i) {
    PoolThread t;
    t.g = (int)(i % q.G);
    long r = i / q.G;
    const int wx = (int)(r % q.Wc);
    r /= q.Wc;
    const int wy = (int)(r % q.Hc);
    const long b = r / q.Hc;
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * wy + k / 2, x = 2 * wx + k % 2;
        t.in_pix[k] = (y < q.H && x < q.W) ? (b * q.H + y) * q.W + x : -1;
    }
    t.out_pix = (wy < q.Ho && wx < q.Wo) ? (b * q.Ho + wy) * q.Wo + wx : -1;
    return t;
}

VT_HD long blocks_for(long threads) { return (threads + kBlock - 1) / kBlock; }

}  // namespace vt
