// The 64-lane backend of the bit-sliced decoders' CPU emulators (tests/c/bitslice*_emu.cpp): a "wave register" is an array of 64
// lanes, the cross-lane / LDS / memory operations are plain loops -- the operations of labrador_ldpc_amd/csrc/hip_backend.hpp -- and
// every address the kernel text forms is CHECKED.  A failed check throws; the emulators' extern "C" entries turn that into return
// value 1, and every test asserts 0.
//   LDS: bounds against exactly the layout size the driver passes; 4-byte alignment of lds_write32, 16-byte alignment of lds_read128 /
//        lds_write128
//   global: 16-byte alignment of gstore128; every gload128 inside the window [lo, hi) the driver sets from its rows (GlobalWindow).
//        No window set: a fault.  (The bit-flipping text, decode_bf_bitslice.hpp, has no gload128: its driver sets none.)
// Plain C++: the f32 loader's quantiser, which needs llr_quantise.hpp and the HIP headers, is in the two emulators that read f32.
#pragma once

#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

namespace {

struct Vec {
    uint32_t l[64];
};

struct EmuBackend {
    using V = Vec;
    // the workgroup's LDS (bounds-checked) and this wave's base in it: the two waves of a split group share one store
    std::shared_ptr<std::vector<uint8_t>> store;
    size_t base = 0;
    explicit EmuBackend(size_t lds_bytes) : store(std::make_shared<std::vector<uint8_t>>(lds_bytes, 0xA5)) {}
    EmuBackend(std::shared_ptr<std::vector<uint8_t>> shared, size_t base_) : store(std::move(shared)), base(base_) {}
    struct Lds {
        std::vector<uint8_t> *v; size_t base;
        uint8_t &at(size_t a) const { return v->at(base + a); }
    };
    Lds lds_() const { return Lds{store.get(), base}; }

    template <class F> static V map1(const V &a, F f) { V r; for (int i = 0; i < 64; ++i) r.l[i] = f(a.l[i]); return r; }
    template <class F> static V map2(const V &a, const V &b, F f) { V r; for (int i = 0; i < 64; ++i) r.l[i] = f(a.l[i], b.l[i]); return r; }

    static void fence() {}
    static void lds_wait() {}
    static void mem_fence() {}
    static void pin(V &) {}
    static V c(uint32_t x) { V r; for (auto &e : r.l) e = x; return r; }
    V lane() const { V r; for (int i = 0; i < 64; ++i) r.l[i] = (uint32_t)i; return r; }
    template <int TT> static V bitop3(const V &a, const V &b, const V &cc)
    {
        V r;
        for (int i = 0; i < 64; ++i) {
            uint32_t o = 0;
            for (int m = 0; m < 8; ++m)
                if ((TT >> m) & 1) o |= ((m & 4) ? a.l[i] : ~a.l[i]) & ((m & 2) ? b.l[i] : ~b.l[i]) & ((m & 1) ? cc.l[i] : ~cc.l[i]);
            r.l[i] = o;
        }
        return r;
    }
    static V and_(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x & y; }); }
    static V or_(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x | y; }); }
    static V xor_(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x ^ y; }); }
    static V andn(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x & ~y; }); }
    static V not_(const V &a) { return map1(a, [](uint32_t x) { return ~x; }); }
    static V add(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x + y; }); }
    static V sub(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x - y; }); }
    static V mul_u(const V &a, uint32_t k) { return map1(a, [k](uint32_t x) { return x * k; }); }
    static V shl(const V &a, int s) { return map1(a, [s](uint32_t x) { return x << s; }); }
    static V shr(const V &a, int s) { return map1(a, [s](uint32_t x) { return x >> s; }); }
    static V sar(const V &a, int s) { return map1(a, [s](uint32_t x) { return (uint32_t)((int32_t)x >> s); }); }
    static V shl_v(const V &a, const V &s) { return map2(a, s, [](uint32_t x, uint32_t y) { return x << (y & 31); }); }
    static V shr_v(const V &a, const V &s) { return map2(a, s, [](uint32_t x, uint32_t y) { return x >> (y & 31); }); }
    static V bfe(const V &v, const V &off, int width) { return map2(v, off, [width](uint32_t x, uint32_t o) { return (x >> (o & 31)) & ((1u << width) - 1); }); }
    static V rotr(const V &x, const V &amt) { return map2(x, amt, [](uint32_t v, uint32_t a) { a &= 31; return a ? (v >> a) | (v << (32 - a)) : v; }); }
    static V less_u(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x < y ? 0xFFFFFFFFu : 0u; }); }
    static V eq(const V &a, const V &b) { return map2(a, b, [](uint32_t x, uint32_t y) { return x == y ? 0xFFFFFFFFu : 0u; }); }
    template <int CTRL> static V quad_perm(const V &x) { V r; for (int i = 0; i < 64; ++i) r.l[i] = x.l[(i & ~3) | ((CTRL >> (2 * (i & 3))) & 3)]; return r; }
    V bperm(const V &addr, const V &x) const { V r; for (int i = 0; i < 64; ++i) r.l[i] = x.l[(addr.l[i] >> 2) & 63]; return r; }

    // ---- LDS
    V lds_read32(const V &addr) const { V r; for (int i = 0; i < 64; ++i) std::memcpy(&r.l[i], &lds_().at(addr.l[i]), 4), (void)lds_().at(addr.l[i] + 3); return r; }
    void lds_write32(const V &addr, const V &v)
    {
        for (int i = 0; i < 64; ++i) {
            if (addr.l[i] % 4) throw std::runtime_error("ds_write_b32 at an address that is not 4-byte aligned");
            (void)lds_().at(addr.l[i] + 3);
            std::memcpy(&lds_().at(addr.l[i]), &v.l[i], 4);
        }
    }
    void lds_write32_if(const V &addr, const V &v, const V &pred) { for (int i = 0; i < 64; ++i) if (pred.l[i]) { (void)lds_().at(addr.l[i] + 3); std::memcpy(&lds_().at(addr.l[i]), &v.l[i], 4); } }
    V lds_read_u16(const V &addr) const { V r; for (int i = 0; i < 64; ++i) r.l[i] = lds_().at(addr.l[i]) | (uint32_t)lds_().at(addr.l[i] + 1) << 8; return r; }
    void lds_write16(const V &addr, const V &v) { for (int i = 0; i < 64; ++i) { lds_().at(addr.l[i]) = (uint8_t)v.l[i]; lds_().at(addr.l[i] + 1) = (uint8_t)(v.l[i] >> 8); } }
    V lds_read_u8(const V &addr) const { V r; for (int i = 0; i < 64; ++i) r.l[i] = lds_().at(addr.l[i]); return r; }
    void lds_write8(const V &addr, const V &v) { for (int i = 0; i < 64; ++i) lds_().at(addr.l[i]) = (uint8_t)v.l[i]; }
    void lds_read128(const V &addr, V (&w)[4]) const
    {
        for (int i = 0; i < 64; ++i) {
            if (addr.l[i] % 16) throw std::runtime_error("ds_read_b128 at an address that is not 16-byte aligned");
            for (int k = 0; k < 4; ++k) { (void)lds_().at(addr.l[i] + 4 * k + 3); std::memcpy(&w[k].l[i], &lds_().at(addr.l[i] + 4 * k), 4); }
        }
    }
    void lds_write128(const V &addr, const V (&w)[4])
    {
        for (int i = 0; i < 64; ++i) {
            if (addr.l[i] % 16) throw std::runtime_error("ds_write_b128 at an address that is not 16-byte aligned");
            for (int k = 0; k < 4; ++k) { (void)lds_().at(addr.l[i] + 4 * k + 3); std::memcpy(&lds_().at(addr.l[i] + 4 * k), &w[k].l[i], 4); }
        }
    }

    // ---- global memory
    static V gload32(const void *p, const V &off, const V &pred)
    {
        V r;
        for (int i = 0; i < 64; ++i) { r.l[i] = 0; if (pred.l[i]) std::memcpy(&r.l[i], (const char *)p + off.l[i], 4); }
        return r;
    }
    static V gload32(const void *p, const V &off) { V r; for (int i = 0; i < 64; ++i) std::memcpy(&r.l[i], (const char *)p + off.l[i], 4); return r; }
    // every 16-byte global load must lie inside the rows the caller handed over: the loaders' lanes of codewords beyond the batch read
    // the group's first frame, idle lanes repeat a frame's last 16 bytes, never memory behind the batch
    static inline const char *lo = nullptr, *hi = nullptr;
    static void gload128(const void *p, const V &off, V (&w)[4])
    {
        for (int i = 0; i < 64; ++i) {
            const char *at = (const char *)p + off.l[i];
            if (at < lo || at + 16 > hi) throw std::runtime_error("16-byte global load outside the batch's rows");
            for (int k = 0; k < 4; ++k) std::memcpy(&w[k].l[i], at + 4 * k, 4);
        }
    }
    static void gstore128(void *p, const V &off, const V (&w)[4], const V &pred)
    {
        for (int i = 0; i < 64; ++i) {
            if (!pred.l[i]) continue;
            if (((uintptr_t)p + off.l[i]) % 16) throw std::runtime_error("16-byte global store at an address that is not 16-byte aligned");
            for (int k = 0; k < 4; ++k) std::memcpy((char *)p + off.l[i] + 4 * k, &w[k].l[i], 4);
        }
    }
    static void gstore32(void *p, const V &off, const V &v, const V &pred) { for (int i = 0; i < 64; ++i) if (pred.l[i]) std::memcpy((char *)p + off.l[i], &v.l[i], 4); }
    static void gstore32_stream(void *p, const V &off, const V &v, const V &pred) { for (int i = 0; i < 64; ++i) if (pred.l[i]) std::memcpy((char *)p + off.l[i], &v.l[i], 4); }
    static void gstore8(void *p, const V &off, const V &v, const V &pred) { for (int i = 0; i < 64; ++i) if (pred.l[i]) ((uint8_t *)p)[off.l[i]] = (uint8_t)v.l[i]; }

    static V select_lanes(uint64_t m, const V &a, const V &b) { V r; for (int i = 0; i < 64; ++i) r.l[i] = ((m >> i) & 1) ? a.l[i] : b.l[i]; return r; }
    static uint32_t readlane(const V &x, int l) { return x.l[l & 63]; }
    static uint64_t ballot(const V &x) { uint64_t m = 0; for (int i = 0; i < 64; ++i) m |= (uint64_t)(x.l[i] != 0) << i; return m; }
    static V plane_of(uint64_t m) { V r; for (int i = 0; i < 64; ++i) r.l[i] = ((m >> i) & 1) ? 0xFFFFFFFFu : 0u; return r; }
};

// the window of gload128 for the time of one driver call: `batch` rows of `row` elements at `rows`
struct GlobalWindow {
    template <class T>
    GlobalWindow(const T *rows, size_t batch, size_t row)
    {
        EmuBackend::lo = (const char *)rows;
        EmuBackend::hi = (const char *)(rows + batch * row);
    }
    ~GlobalWindow() { EmuBackend::lo = EmuBackend::hi = nullptr; }
    GlobalWindow(const GlobalWindow &) = delete;
    GlobalWindow &operator=(const GlobalWindow &) = delete;
};

// an extern "C" decode entry's body: a fault of the backend (std::out_of_range of the LDS store, the runtime_errors above) -> 1
template <class F>
int faults_to_1(F &&f)
{
    try {
        return f();
    } catch (const std::exception &) {
        return 1;
    }
}

}  // namespace
