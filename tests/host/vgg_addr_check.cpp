// Host-side address check of the VGG16 stage-1 kernels (csrc/vgg_train.hip): walks the whole
// launch grid of the ReLU backward (+ its final reduction) and of the MaxPool2d(2, 2)
// backward with the index functions the kernels themselves use (csrc/vgg_train_addr.h) and
// asserts offset + access bytes <= buffer bytes for every access of every thread, over the
// full VGG16 layer ladder at 36x44, 64x64 and 224x224 (B = 1) and a few odd shapes, in both
// layout pairs (gradients S3 / activations S2, and S1 / S1).  Each access also touches its
// first and last byte in a buffer of exactly the size the trainer allocates, so a build with
// -fsanitize=address,undefined checks the same thing independently; and every output group
// must be written exactly once.  A plain executable: exit status 0 = all checks passed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tcam_wsol_video_amd/csrc/vgg_train_addr.h"

namespace {

long g_accesses = 0;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

struct Buf {
    std::vector<uint8_t> mem;
    explicit Buf(size_t n) : mem(n) {}
    void touch(long off, long bytes, const char* what) {
        if (off < 0 || bytes <= 0 || (size_t)(off + bytes) > mem.size()) {
            std::fprintf(stderr, "out of bounds: %s offset %ld + %ld > %zu\n", what, off, bytes,
                         mem.size());
            std::exit(1);
        }
        mem[(size_t)off] ^= 1;
        mem[(size_t)(off + bytes - 1)] ^= 1;
        ++g_accesses;
    }
};

// relu_bwd_kernel + relu_bwd_final_kernel at (P, C), groups of gbg (gradient) / gba
// (activation) bytes
void walk_relu(long P, int C, int gbg, int gba) {
    vt::ReluGeom q;
    CHECK(vt::relu_geom(P, C, &q));
    CHECK(q.per >= 1 && q.per * q.G <= vt::kBlock && q.blocks >= 1 && q.blocks <= vt::kMaxBlocks);
    Buf dout((size_t)P * q.G * gbg), out((size_t)P * q.G * gba), dz((size_t)P * q.G * gbg);
    Buf part(vt::relu_ws_bytes(q)), amax((size_t)C * 4), db((size_t)C * 4);
    std::vector<uint8_t> written((size_t)P * q.G, 0);
    std::vector<uint8_t> part_written((size_t)q.blocks * C, 0), db_written((size_t)C, 0);
    for (int b = 0; b < q.blocks; ++b) {
        for (int tid = 0; tid < vt::kBlock; ++tid) {
            const vt::ReluThread t = vt::relu_thread(q, b, tid);
            CHECK(t.g >= 0 && t.g < q.G && t.step > 0);
            if (t.p0 >= 0) {
                for (long p = t.p0; p < q.P; p += t.step) {
                    dout.touch(vt::group_off(p, q.G, t.g, gbg), gbg, "relu dout");
                    out.touch(vt::group_off(p, q.G, t.g, gba), gba, "relu out");
                    dz.touch(vt::group_off(p, q.G, t.g, gbg), gbg, "relu dz");
                    ++written[(size_t)(p * q.G + t.g)];
                }
            }
            // the block reduction: channels tid, tid + kBlock, ... read rows r < per from the
            // kBlock * 8 LDS slots (slot tid * 8 + e is thread tid's) and write their partial
            for (int c = tid; c < q.G * 8; c += vt::kBlock) {
                for (int r = 0; r < q.per; ++r) {
                    const int slot = vt::relu_lds_slot(q, r, c);
                    CHECK(slot >= 0 && slot < vt::kBlock * 8);
                    CHECK(slot / 8 == r * q.G + c / 8 && slot / 8 < q.per * q.G);
                }
                part.touch(vt::relu_part_off(q, b, c), 8, "relu partial sums");
                amax.touch((long)c * 4, 4, "relu amax");
                ++part_written[(size_t)b * C + c];
            }
        }
    }
    for (uint8_t w : written) CHECK(w == 1);
    for (uint8_t w : part_written) CHECK(w == 1);   // every (block, channel) sum exists
    const long fb = vt::blocks_for(C);
    for (long b = 0; b < fb; ++b)
        for (int tid = 0; tid < vt::kBlock; ++tid) {
            const long c = b * vt::kBlock + tid;
            if (c >= q.G * 8) continue;
            for (int k = 0; k < q.blocks; ++k)
                part.touch(vt::relu_part_off(q, k, (int)c), 8, "relu final partial");
            db.touch(c * 4, 4, "relu db");
            ++db_written[(size_t)c];
        }
    for (uint8_t w : db_written) CHECK(w == 1);
}

// maxpool2x2_bwd_kernel at (B, C, H, W)
void walk_pool(int B, int C, int H, int W, int gbg, int gba) {
    vt::PoolGeom q;
    CHECK(vt::pool_geom(B, C, H, W, H / 2, W / 2, &q));
    Buf gout((size_t)B * q.Ho * q.Wo * q.G * gbg), x((size_t)B * H * W * q.G * gba);
    Buf gin((size_t)B * H * W * q.G * gbg);
    std::vector<uint8_t> written((size_t)B * H * W * q.G, 0);
    const long nb = vt::blocks_for(q.total);
    for (long b = 0; b < nb; ++b)
        for (int tid = 0; tid < vt::kBlock; ++tid) {
            const long i = b * vt::kBlock + tid;
            if (i >= q.total) continue;
            const vt::PoolThread t = vt::pool_thread(q, i);
            CHECK(t.g >= 0 && t.g < q.G);
            for (int k = 0; k < 4; ++k) {
                if (t.out_pix >= 0) CHECK(t.in_pix[k] >= 0);   // a full window is in the frame
                if (t.in_pix[k] < 0) continue;
                if (t.out_pix >= 0) x.touch(vt::group_off(t.in_pix[k], q.G, t.g, gba), gba, "pool x");
                gin.touch(vt::group_off(t.in_pix[k], q.G, t.g, gbg), gbg, "pool gin");
                ++written[(size_t)(t.in_pix[k] * q.G + t.g)];
            }
            if (t.out_pix >= 0) gout.touch(vt::group_off(t.out_pix, q.G, t.g, gbg), gbg, "pool gout");
        }
    for (uint8_t w : written) CHECK(w == 1);
}

// encoders/vgg.py:47-58 (WSOL16) + conv6; 0 = MaxPool2d(2, 2)
const int kLadder[] = {64, 64, 0, 128, 128, 0, 256, 256, 256, 0, 512, 512, 512, 512, 512, 512, 1024};

void walk_ladder(int B, int H, int W) {
    const int pairs[2][2] = {{48, 32}, {16, 16}};
    int C = 0;
    for (int v : kLadder) {
        for (const auto& gb : pairs) {
            if (v) {
                walk_relu((long)B * H * W, v, gb[0], gb[1]);
            } else {
                CHECK(H >= 2 && W >= 2);
                walk_pool(B, C, H, W, gb[0], gb[1]);
            }
        }
        if (v) {
            C = v;
        } else {
            H /= 2;
            W /= 2;
        }
    }
}

}  // namespace

int main() {
    walk_ladder(1, 36, 44);
    walk_ladder(1, 64, 64);
    walk_ladder(1, 224, 224);
    // odd sizes, channel counts whose group count does not divide the block, one pixel row
    // per block (G = 256), more pixels than the fixed grid covers in one pass
    const int pairs[2][2] = {{48, 32}, {16, 16}};
    for (const auto& gb : pairs) {
        walk_relu(2 * 9 * 11, 8, gb[0], gb[1]);
        walk_relu(2 * 9 * 11, 24, gb[0], gb[1]);
        walk_relu(3 * 7 * 5, 2048, gb[0], gb[1]);
        walk_relu(1, 8, gb[0], gb[1]);
        walk_relu(40000, 72, gb[0], gb[1]);
        walk_pool(2, 8, 6, 10, gb[0], gb[1]);
        walk_pool(2, 64, 9, 11, gb[0], gb[1]);
        walk_pool(1, 24, 2, 3, gb[0], gb[1]);
        walk_pool(3, 8, 3, 2, gb[0], gb[1]);
    }
    // geometries the entries refuse
    vt::ReluGeom rq;
    vt::PoolGeom pq;
    CHECK(!vt::relu_geom(10, 12, &rq) && !vt::relu_geom(0, 8, &rq) && !vt::relu_geom(10, 2056, &rq));
    CHECK(!vt::pool_geom(1, 12, 4, 4, 2, 2, &pq) && !vt::pool_geom(1, 8, 5, 4, 3, 2, &pq));
    CHECK(!vt::pool_geom(1, 8, 4, 5, 2, 3, &pq) && !vt::pool_geom(1, 8, 1, 4, 0, 2, &pq));
    std::printf("vgg_addr_check: ok, %ld accesses checked\n", g_accesses);
    return 0;
}
