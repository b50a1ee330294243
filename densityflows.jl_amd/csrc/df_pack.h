// df_pack.h — host-only helpers of the weight packers (df_plan.cpp; the fragment walkers
// also serve the training blobs of df_train_plan.cpp): cutting a blob into stages, writing
// a parameter together with its repack pair, and the index nests of the MFMA fragments.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "df_plan.h"

namespace df {
namespace pack {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Cuts a blob into the stages a kernel copies whole into LDS.  Two ways to fill it:
//   alloc(bytes)        fill-to-capacity stages: reserves room in the open stage, opening a
//                       new one when it does not fit; close() pads the open stage to the DMA
//                       granularity (kStageAlign) and records its size in stage_max
//   fixed_stage(bytes)  one stage of exactly `bytes` (the wide blobs)
class StageWriter {
public:
    struct Slot {
        int stage, off;  // stage id, byte offset in the stage
        int64_t at;      // byte offset in the blob
    };

    StageWriter(std::vector<uint8_t>& blob, std::vector<DevStage>& stages, int* stage_max = nullptr, int cap = 0)
        : blob_(blob), stages_(stages), stage_max_(stage_max), cap_(cap) {}

    int cap() const { return cap_; }
    int remaining() const { return cur_ < 0 ? 0 : cap_ - used_; }

    void begin_stage() {
        close();
        cur_ = (int)stages_.size();
        DevStage s{};
        s.src_off = (int64_t)blob_.size();
        stages_.push_back(s);
        used_ = 0;
    }

    // bytes: a multiple of 16, at most cap()
    Slot alloc(int bytes) {
        if (cur_ < 0 || used_ + bytes > cap_) begin_stage();
        const int off = used_;
        used_ += bytes;
        blob_.resize((size_t)stages_[cur_].src_off + used_, 0);
        return {cur_, off, stages_[cur_].src_off + off};
    }

    // returns the stage's byte offset in the blob
    int64_t fixed_stage(int bytes) {
        DevStage s{};
        s.src_off = (int64_t)blob_.size();
        s.bytes = bytes;
        stages_.push_back(s);
        blob_.resize(blob_.size() + bytes, 0);
        return s.src_off;
    }

    void close() {
        if (cur_ < 0) return;
        used_ = round_up(used_, kStageAlign);
        blob_.resize((size_t)stages_[cur_].src_off + used_, 0);
        stages_[cur_].bytes = used_;
        if (stage_max_) *stage_max_ = std::max(*stage_max_, used_);
    }

private:
    std::vector<uint8_t>& blob_;
    std::vector<DevStage>& stages_;
    int* stage_max_;
    int cap_;
    int cur_ = -1;
    int used_ = 0;
};

// A value of the descriptor and its index in Plan::trainables (src < 0: not a parameter,
// a zero of the padding).
struct Param {
    int32_t src;
    float v;
};

// The parameters of one blob: writes a value at a byte offset and appends the pair
// (destination ← source) the device-side repack kernel walks, in the order of the calls.
//   WORDS   f32 blobs:   float index  ← trainables index
//   PLANES  bf16x3 blobs: byte offset ← trainables index·4 + plane (plane 3: the f32 itself)
template <class T>
class ParamSink {
public:
    enum Unit { WORDS, PLANES };

    ParamSink(std::vector<T>& blob, std::vector<int32_t>& dst, std::vector<int32_t>& src, Unit unit)
        : blob_(blob), dst_(dst), src_(src), unit_(unit) {}

    void f32(int64_t at, Param p) {
        std::memcpy(bytes() + at, &p.v, 4);
        if (p.src < 0) return;
        if (unit_ == WORDS) record(at / 4, p.src);
        else record(at, p.src * 4 + 3);
    }

    void plane(int64_t at, int plane, Param p) {
        const uint16_t h = bf16_split_plane(p.v, plane);
        std::memcpy(bytes() + at, &h, 2);
        if (p.src >= 0) record(at, p.src * 4 + plane);
    }

private:
    uint8_t* bytes() { return reinterpret_cast<uint8_t*>(blob_.data()); }
    void record(int64_t dst, int32_t src) {
        dst_.push_back((int32_t)dst);
        src_.push_back(src);
    }

    std::vector<T>& blob_;
    std::vector<int32_t>&dst_, &src_;
    Unit unit_;
};

// ---- which input k an MFMA A-fragment entry holds (lane = 16g + i holds row 16m + i) ----
// first Dense, f32: k-step s multiplies the four features 4s + g of the layer's feature
// table (compact layout: s = r < ks; k-quad layout: s = 4kq + r)
// (function objects, so that a walker inlines the order it is given)
constexpr int k_state(int s, int g) { return 4 * s + g; }
constexpr auto k_state_quad = [](int kq, int g, int r) { return k_state(4 * kq + r, g); };
// hidden / output Dense, f32: k-quad kq is input row tile kq, entry r of lane group g its row 4g + r
constexpr auto k_hidden_quad = [](int kq, int g, int r) { return 16 * kq + 4 * g + r; };
// bf16 planes, hidden / output Dense: chunk c is the accumulator tiles 2c, 2c + 1 (e >> 2), rows as above
constexpr auto k_plane_hidden = [](int c, int g, int e) { return 32 * c + 16 * (e >> 2) + 4 * g + (e & 3); };
// bf16 planes, first Dense of the wide SPLIT kernel: features through the layer's split table
constexpr auto k_plane_first = [](int c, int g, int e) { return 32 * c + 8 * g + e; };

// f32 fragments [kq - kq0][m < mt][lane][4]: fn(float index in the fragments, row, k_of(kq, g, r))
template <class K, class F>
void for_each_f32_frag(int kq0, int kq1, int mt, K k_of, F fn) {
    for (int kq = kq0; kq < kq1; ++kq)
        for (int m = 0; m < mt; ++m)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r)
                    fn(((int64_t)((kq - kq0) * mt + m) * 64 + lane) * 4 + r, 16 * m + (lane & 15),
                       k_of(kq, lane >> 4, r));
}

// bf16x3 fragments [c - c0][m < mt][plane < 3][lane][8] of row tiles m0 + m:
// fn(byte offset in the fragments, row, k_of(c, g, e), plane)
template <class K, class F>
void for_each_plane_frag(int c0, int c1, int m0, int mt, K k_of, F fn) {
    for (int c = c0; c < c1; ++c)
        for (int m = 0; m < mt; ++m)
            for (int p = 0; p < 3; ++p)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e)
                        fn(((((int64_t)(c - c0) * mt + m) * 3 + p) * 64 + lane) * 16 + 2 * e,
                           16 * (m0 + m) + (lane & 15), k_of(c, lane >> 4, e), p);
}

}  // namespace pack
}  // namespace df
