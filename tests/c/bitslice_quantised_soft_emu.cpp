// CPU emulation of the bit-sliced i8 decoder READING F32 LLRs WITH soft output (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp,
// decode_group<..., SOFT = true, QuantisedF32>, plain and CORRECTED = true at MULBITS 0 / 4 / 8): the SAME source text
// the gfx950 kernels of decode_ms_bs_quantised_soft.hip are compiled from -- the f32 loader, the iteration, the correction step, the kept
// planes, store_marginals -- instantiated with a backend whose "wave register" is an array of 64 lanes, whose LDS accessors are
// bounds-checked against exactly Geo::LDS_BYTES_SOFT of the shipped placement and whose 16-byte global loads must stay inside the
// batch's rows.  The quantiser is the library's own (ldpc::quantise_llr of llr_quantise.hpp, compiled here by g++ for the host).  Test
// infrastructure (tests/test_bitslice_quantised_soft_emu.py compares it with the restatements on the CPU); it is not part of the
// product, and it shares no text with the other emulators: the backend below is a copy of its own.
//   g++ -O1 -std=c++20 -fno-fast-math -ffp-contract=off -shared -fPIC -DEMU_CODE=TM8192 -D__HIP_PLATFORM_AMD__ -I<rocm>/include
//       -Ilabrador_ldpc_amd/csrc tests/c/bitslice_quantised_soft_emu.cpp -o build/libbitslice_quantised_soft_emu_TM8192.so
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#define BS_FN inline
#include "decode_ms_bitslice.hpp"
#include "llr_quantise.hpp"

namespace {

struct Vec {
    uint32_t l[64];
};

struct EmuBackend {
    using V = Vec;
    // the workgroup's LDS (bounds-checked) and this wave's base in it
    std::shared_ptr<std::vector<uint8_t>> store;
    size_t base = 0;
    explicit EmuBackend(size_t lds_bytes) : store(std::make_shared<std::vector<uint8_t>>(lds_bytes, 0xA5)) {}
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
    V lds_read32(const V &addr) const { V r; for (int i = 0; i < 64; ++i) std::memcpy(&r.l[i], &lds_().at(addr.l[i]), 4), (void)lds_().at(addr.l[i] + 3); return r; }
    void lds_write32(const V &addr, const V &v)
    {
        for (int i = 0; i < 64; ++i) {
            if (addr.l[i] % 4) throw std::runtime_error("ds_write_b32 at an address that is not 4-byte aligned");
            (void)lds_().at(addr.l[i] + 3);
            std::memcpy(&lds_().at(addr.l[i]), &v.l[i], 4);
        }
    }
    V lds_read_u16(const V &addr) const { V r; for (int i = 0; i < 64; ++i) r.l[i] = lds_().at(addr.l[i]) | (uint32_t)lds_().at(addr.l[i] + 1) << 8; return r; }
    void lds_write16(const V &addr, const V &v) { for (int i = 0; i < 64; ++i) { lds_().at(addr.l[i]) = (uint8_t)v.l[i]; lds_().at(addr.l[i] + 1) = (uint8_t)(v.l[i] >> 8); } }
    void lds_write32_if(const V &addr, const V &v, const V &pred) { for (int i = 0; i < 64; ++i) if (pred.l[i]) { (void)lds_().at(addr.l[i] + 3); std::memcpy(&lds_().at(addr.l[i]), &v.l[i], 4); } }
    V lds_read_u8(const V &addr) const { V r; for (int i = 0; i < 64; ++i) r.l[i] = lds_().at(addr.l[i]); return r; }
    void lds_write8(const V &addr, const V &v) { for (int i = 0; i < 64; ++i) lds_().at(addr.l[i]) = (uint8_t)v.l[i]; }
    void lds_read128(const V &addr, V (&w)[4]) const
    {
        for (int i = 0; i < 64; ++i) {
            if (addr.l[i] % 16) throw std::runtime_error("ds_read_b128 at an address that is not 16-byte aligned");
            for (int k = 0; k < 4; ++k) { (void)lds_().at(addr.l[i] + 4 * k + 3); std::memcpy(&w[k].l[i], &lds_().at(addr.l[i] + 4 * k), 4); }
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
    static V gload32(const void *p, const V &off, const V &pred)
    {
        V r;
        for (int i = 0; i < 64; ++i) { r.l[i] = 0; if (pred.l[i]) std::memcpy(&r.l[i], (const char *)p + off.l[i], 4); }
        return r;
    }
    static V gload32(const void *p, const V &off) { V r; for (int i = 0; i < 64; ++i) std::memcpy(&r.l[i], (const char *)p + off.l[i], 4); return r; }
    // every 16-byte global load must lie inside the rows the caller handed over ([lo, hi), set by run()): the loader's lanes of
    // codewords beyond the batch read the group's first frame, never memory behind the batch
    static inline const char *lo = nullptr, *hi = nullptr;
    static void gload128(const void *p, const V &off, V (&w)[4])
    {
        for (int i = 0; i < 64; ++i) {
            const char *at = (const char *)p + off.l[i];
            if (at < lo || at + 16 > hi) throw std::runtime_error("16-byte global load outside the batch's rows");
            for (int k = 0; k < 4; ++k) std::memcpy(&w[k].l[i], at + 4 * k, 4);
        }
    }
    // four f32 LLRs (their bits) -> one dword of four i8 bytes by the library's one rule
    static V quantise4_i8(const V (&w)[4], float scale, float lim)
    {
        V r;
        for (int i = 0; i < 64; ++i) {
            uint32_t o = 0;
            for (int k = 0; k < 4; ++k) {
                float x;
                std::memcpy(&x, &w[k].l[i], 4);
                o |= (uint32_t)(uint8_t)ldpc::quantise_llr<int8_t>(x, scale, lim) << (8 * k);
            }
            r.l[i] = o;
        }
        return r;
    }
    void lds_write128(const V &addr, const V (&w)[4])
    {
        for (int i = 0; i < 64; ++i) {
            if (addr.l[i] % 16) throw std::runtime_error("ds_write_b128 at an address that is not 16-byte aligned");
            for (int k = 0; k < 4; ++k) { (void)lds_().at(addr.l[i] + 4 * k + 3); std::memcpy(&lds_().at(addr.l[i] + 4 * k), &w[k].l[i], 4); }
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

// the one-wave lockstep driver, group after group (decode_ms_bsqa_kernel<CODE>, decode_ms_bsqca_kernel<CODE, MULBITS>): the LDS store
// has exactly the soft layout's size, so an address beyond it throws here
template <int CODE, bool CORRECTED, int MULBITS, class SRC>
int run(const typename SRC::T *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters,
        uint32_t scale_num, uint32_t scale_shift, uint32_t offset, SRC source)
{
    using GEO = ldpc::bs::Geo<CODE>;
    EmuBackend::lo = (const char *)llrs;
    EmuBackend::hi = (const char *)(llrs + batch * GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        EmuBackend b(GEO::LDS_BYTES_SOFT);
        ldpc::bs::init_kernel<CODE, EmuBackend>(b);
        ldpc::bs::decode_group<CODE, EmuBackend, CORRECTED, MULBITS, true, SRC>(b, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g,
                                                                                scale_num, scale_shift, offset, app, source);
    }
    return 0;
}

template <class SRC>
int run_form(const typename SRC::T *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters,
             uint32_t scale_num, uint32_t scale_shift, uint32_t offset, int mulbits, SRC source)
{
    if (mulbits >= 0 && (scale_shift > 8 || ldpc::bs::correction_mulbits(scale_num, scale_shift) > mulbits)) return 2;
    try {
        switch (mulbits) {
            case -1: return run<ldpc::EMU_CODE, false, 8, SRC>(llrs, app, out, iters, ok, batch, maxiters, 1, 0, 0, source);
            case 0: return run<ldpc::EMU_CODE, true, 0, SRC>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, source);
            case 4: return run<ldpc::EMU_CODE, true, 4, SRC>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, source);
            case 8: return run<ldpc::EMU_CODE, true, 8, SRC>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, source);
            default: return 2;
        }
    } catch (const std::exception &) {
        return 1;
    }
}

}  // namespace

// One code per shared object (-DEMU_CODE=TM8192 ...): the instantiations compile in parallel (tests/test_bitslice_quantised_soft_emu.py).
#ifndef EMU_CODE
#error "compile with -DEMU_CODE=<TM1536|TM2048|TM6144|TM8192>"
#endif
static_assert(ldpc::bs::bitsliced_soft_code(ldpc::EMU_CODE), "the f32 loader and the soft form exist for the one-wave codes");
extern "C" int bsqa_emu_mulbits(uint32_t scale_num, uint32_t scale_shift) { return ldpc::bs::correction_mulbits(scale_num, scale_shift); }
// The soft decoder on f32 rows at (scale, lim): app [batch][n + p] i8 beside the three hard results.  mulbits < 0: the plain form
// (decode_ms_bsqa_kernel); else the corrected form built for `mulbits` multiplier bits (0, 4, 8; the triple must fit the form).
// 1: an LDS, alignment or global-bounds fault of the kernel text; 2: no such form, or the triple does not fit it
extern "C" int bsqa_emu_decode(const float *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters,
                               float scale, float lim, uint32_t scale_num, uint32_t scale_shift, uint32_t offset, int mulbits)
{
    return run_form(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, mulbits, ldpc::bs::QuantisedF32{scale, lim});
}
// the i8-source soft decoder of the same header in the same forms (decode_ms_bsa_kernel, decode_ms_bsca_kernel): the default SRC
extern "C" int bsqa_emu_decode_i8(const int8_t *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters,
                                  uint32_t scale_num, uint32_t scale_shift, uint32_t offset, int mulbits)
{
    return run_form(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, mulbits, ldpc::bs::RawI8{});
}
extern "C" int bsqa_emu_group(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::G; }
extern "C" int bsqa_emu_code(void) { return ldpc::EMU_CODE; }
extern "C" int bsqa_emu_planes_in_lds(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::SOFT_LDS ? 1 : 0; }
extern "C" int bsqa_emu_lds_bytes(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::LDS_BYTES_SOFT; }
