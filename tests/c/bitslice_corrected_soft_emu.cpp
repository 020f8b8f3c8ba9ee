// CPU emulation of the bit-sliced i8 decoder WITH normalized / offset check messages AND soft output
// (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp, Decoder<..., CORRECTED = true, MULBITS, SOFT = true>): the SAME source
// text the gfx950 kernels of decode_ms_bs_corrected_soft.hip are compiled from, instantiated with the emulators' 64-lane,
// address-checked backend (tests/c/bitslice_emu_backend.hpp), its LDS bounds-checked against the soft layout's size.  Test
// infrastructure (tests/test_bitslice_corrected_soft_emu.py compares it with the restatement on the CPU); it is not part of the product.
//   g++ -O1 -std=c++20 -shared -fPIC -DEMU_CODE=TM8192 -Ilabrador_ldpc_amd/csrc tests/c/bitslice_corrected_soft_emu.cpp -o build/libbitslice_corrected_soft_emu_TM8192.so
#define BS_FN inline
#include "decode_ms_bitslice.hpp"
#include "decode_ms_bitslice_split.hpp"

#include "bitslice_emu_backend.hpp"

namespace {

// the one-wave lockstep driver, group after group (decode_ms_bsca_kernel<CODE, MULBITS>): the LDS store has exactly the soft layout's
// size, so an address beyond it -- or a layout that is too small for what the kernel text touches -- throws here
template <int CODE, int MULBITS>
int run(const int8_t *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, uint32_t scale_num,
        uint32_t scale_shift, uint32_t offset)
{
    using GEO = ldpc::bs::Geo<CODE>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        EmuBackend b(GEO::LDS_BYTES_SOFT);
        ldpc::bs::init_kernel<CODE, EmuBackend>(b);
        ldpc::bs::decode_group<CODE, EmuBackend, true, MULBITS, true>(b, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g, scale_num,
                                                                      scale_shift, offset, app);
    }
    return 0;
}

}  // namespace

// One code per shared object (-DEMU_CODE=TM8192 ...): the instantiations compile in parallel (tests/test_bitslice_corrected_soft_emu.py).
#ifndef EMU_CODE
#error "compile with -DEMU_CODE=<TM1536|TM2048|TM6144|TM8192>"
#endif
static_assert(ldpc::bs::bitsliced_soft_code(ldpc::EMU_CODE), "the corrected soft form exists for the one-wave codes");
// the form the launcher picks for a scale (launch_corrected_soft_in_unit)
extern "C" int bsca_emu_mulbits(uint32_t scale_num, uint32_t scale_shift) { return ldpc::bs::correction_mulbits(scale_num, scale_shift); }
// the corrected soft decoder in the form built for `mulbits` multiplier bits (0, 4, 8; the triple must fit the form: its low
// 8 - mulbits bits of scale_num << (8 - scale_shift) zero): app [batch][n + p] i8 beside the three hard results.
// 1: an LDS, alignment or global-bounds fault of the kernel text; 2: no such form, or the triple does not fit it
extern "C" int bsca_emu_decode(const int8_t *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters,
                               uint32_t scale_num, uint32_t scale_shift, uint32_t offset, int mulbits)
{
    if (scale_shift > 8 || ldpc::bs::correction_mulbits(scale_num, scale_shift) > mulbits) return 2;
    return faults_to_1([&] {
        switch (mulbits) {
            case 0: return run<ldpc::EMU_CODE, 0>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset);
            case 4: return run<ldpc::EMU_CODE, 4>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset);
            case 8: return run<ldpc::EMU_CODE, 8>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset);
            default: return 2;
        }
    });
}
extern "C" int bsca_emu_group(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::G; }
extern "C" int bsca_emu_code(void) { return ldpc::EMU_CODE; }
extern "C" int bsca_emu_planes_in_lds(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::SOFT_LDS ? 1 : 0; }
extern "C" int bsca_emu_lds_bytes(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::LDS_BYTES_SOFT; }
