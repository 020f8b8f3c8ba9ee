// CPU emulation of the bit-sliced i8 decoder READING PACKED HARD DECISIONS (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp,
// load_column_planes<..., PackedHard>, plain and Decoder<..., CORRECTED = true, MULBITS>): the SAME source text the
// gfx950 kernels of decode_ms_bs_hard.hip are compiled from, instantiated with the emulators' 64-lane, address-checked backend
// (tests/c/bitslice_emu_backend.hpp) behind a wrapper that checks the packed loader's 4-byte global loads as well.  Test infrastructure
// (tests/test_bitslice_hard_emu.py compares it with the statements on the CPU); it is not part of the product.
//   g++ -O1 -std=c++20 -shared -fPIC -DEMU_CODE=TM8192 -Ilabrador_ldpc_amd/csrc tests/c/bitslice_hard_emu.cpp
//       -o build/libbitslice_hard_emu_TM8192.so
#define BS_FN inline
#include "decode_ms_bitslice.hpp"

#include "bitslice_emu_backend.hpp"

namespace {

// The shared backend checks its 16-byte global loads only.  The packed loader reads one dword per lane from two arrays: every such
// load must be 4-byte aligned relative to its row pointer and lie inside [0, batch * n / 8) of THE ARRAY IT IS MADE THROUGH: the
// window is the one of `input` and `erasures` that holds the load's base pointer (a group's first row), so a load through `input`
// that lands in `erasures`, or the reverse, is a fault like any other.
struct HardBackend : EmuBackend {
    using EmuBackend::EmuBackend;
    struct Rows { const char *lo, *hi; };
    static inline Rows rows[2] = {};
    static V gload32(const void *p, const V &off)
    {
        const Rows *window = nullptr;
        for (const Rows &r : rows)
            if (r.lo && (const char *)p >= r.lo && (const char *)p < r.hi) window = &r;
        if (!window) throw std::runtime_error("4-byte global load through a pointer outside the batch's packed rows");
        for (int i = 0; i < 64; ++i) {
            const char *at = (const char *)p + off.l[i];
            if (off.l[i] % 4) throw std::runtime_error("4-byte global load at an offset that is not 4-byte aligned");
            if (at < window->lo || at + 4 > window->hi) throw std::runtime_error("4-byte global load outside the rows of the array it is made through");
        }
        return EmuBackend::gload32(p, off);
    }
};
struct HardWindow {
    HardWindow(const uint8_t *input, const uint8_t *erasures, size_t batch, size_t row)
    {
        HardBackend::rows[0] = {(const char *)input, (const char *)input + batch * row};
        HardBackend::rows[1] = erasures ? HardBackend::Rows{(const char *)erasures, (const char *)erasures + batch * row} : HardBackend::Rows{};
    }
    ~HardWindow() { HardBackend::rows[0] = HardBackend::rows[1] = {}; }
    HardWindow(const HardWindow &) = delete;
    HardWindow &operator=(const HardWindow &) = delete;
};

// the one-wave lockstep driver, group after group (decode_ms_bsh_kernel<CODE>, decode_ms_bshc_kernel<CODE, MULBITS>): the LDS store
// has exactly the layout's size, so an address beyond it throws here
template <int CODE, bool CORRECTED, int MULBITS, class SRC>
int run(const typename SRC::T *rows, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, uint32_t scale_num,
        uint32_t scale_shift, uint32_t offset, SRC source)
{
    using GEO = ldpc::bs::Geo<CODE>;
    GlobalWindow window(rows, batch, SRC::row_len(GEO::N));
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        HardBackend b(GEO::LDS_BYTES);
        ldpc::bs::init_kernel<CODE, HardBackend>(b);
        ldpc::bs::decode_group<CODE, HardBackend, CORRECTED, MULBITS, false, SRC>(b, rows, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g,
                                                                                  scale_num, scale_shift, offset, nullptr, source);
    }
    return 0;
}

}  // namespace

// One code per shared object (-DEMU_CODE=TM8192 ...): the instantiations compile in parallel (tests/test_bitslice_hard_emu.py).
#ifndef EMU_CODE
#error "compile with -DEMU_CODE=<TM1536|TM2048|TM6144|TM8192>"
#endif
static_assert(ldpc::bs::bitsliced_soft_code(ldpc::EMU_CODE), "the packed loader exists for the one-wave codes");
extern "C" int bsh_emu_mulbits(uint32_t scale_num, uint32_t scale_shift) { return ldpc::bs::correction_mulbits(scale_num, scale_shift); }
// The decoder on packed rows at `magnitude`, erasures NULL or packed mask rows.  mulbits < 0: the plain form (decode_ms_bsh_kernel);
// else the corrected form built for `mulbits` multiplier bits (0, 4, 8; the triple must fit the form).  1: an LDS, alignment or
// global-bounds fault of the kernel text; 2: no such form, or the triple does not fit it
extern "C" int bsh_emu_decode(const uint8_t *input, const uint8_t *erasures, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch,
                              uint32_t maxiters, uint32_t magnitude, uint32_t scale_num, uint32_t scale_shift, uint32_t offset, int mulbits)
{
    using ldpc::bs::PackedHard;
    if (mulbits >= 0 && (scale_shift > 8 || ldpc::bs::correction_mulbits(scale_num, scale_shift) > mulbits)) return 2;
    if (magnitude < 1 || magnitude > 127) return 2;
    const PackedHard src{magnitude, erasures};
    HardWindow window(input, erasures, batch, ldpc::bs::Geo<ldpc::EMU_CODE>::N / 8);
    return faults_to_1([&] {
        switch (mulbits) {
            case -1: return run<ldpc::EMU_CODE, false, 8, PackedHard>(input, out, iters, ok, batch, maxiters, 1, 0, 0, src);
            case 0: return run<ldpc::EMU_CODE, true, 0, PackedHard>(input, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, src);
            case 4: return run<ldpc::EMU_CODE, true, 4, PackedHard>(input, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, src);
            case 8: return run<ldpc::EMU_CODE, true, 8, PackedHard>(input, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, src);
            default: return 2;
        }
    });
}
// the i8-source decoder of the same header, plain form (decode_ms_bs_kernel's lockstep text): the default SRC
extern "C" int bsh_emu_decode_i8(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run<ldpc::EMU_CODE, false, 8, ldpc::bs::RawI8>(llrs, out, iters, ok, batch, maxiters, 1, 0, 0, {}); });
}
extern "C" int bsh_emu_group(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::G; }
extern "C" int bsh_emu_code(void) { return ldpc::EMU_CODE; }
extern "C" int bsh_emu_lds_bytes(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::LDS_BYTES; }
