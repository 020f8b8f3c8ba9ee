// CPU emulation of the bit-sliced i8 decoder WITH soft output (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp, Decoder<..., SOFT = true>;
// DESIGN.md 4.16): the SAME source text the gfx950 kernels of decode_ms_bs_soft.hip are compiled from, instantiated with the emulators'
// 64-lane, address-checked backend (tests/c/bitslice_emu_backend.hpp), its LDS bounds-checked against the soft layout's size.  Test
// infrastructure (tests/test_bitslice_soft_emu.py compares it with the oracle on the CPU); it is not part of the product.
//   g++ -O1 -std=c++20 -shared -fPIC -DEMU_CODE=TM8192 -Ilabrador_ldpc_amd/csrc tests/c/bitslice_soft_emu.cpp -o build/libbitslice_soft_emu_TM8192.so
#define BS_FN inline
#include "decode_ms_bitslice.hpp"
#include "decode_ms_bitslice_split.hpp"

#include "bitslice_emu_backend.hpp"

namespace {

// the one-wave lockstep driver, group after group (decode_ms_bsa_kernel): the LDS store has exactly the soft layout's size, so an address
// beyond it -- or a layout that is too small for what the kernel text touches -- throws here
template <int CODE, bool SOFT>
int run(const int8_t *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    using GEO = ldpc::bs::Geo<CODE>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        EmuBackend b(SOFT ? GEO::LDS_BYTES_SOFT : GEO::LDS_BYTES);
        ldpc::bs::init_kernel<CODE, EmuBackend>(b);
        ldpc::bs::decode_group<CODE, EmuBackend, false, 8, SOFT>(b, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g, 1, 0, 0, app);
    }
    return 0;
}

}  // namespace

// One code per shared object (-DEMU_CODE=TM8192 ...): the instantiations compile in parallel (tests/test_bitslice_soft_emu.py).
#ifndef EMU_CODE
#error "compile with -DEMU_CODE=<TM1536|TM2048|TM6144|TM8192>"
#endif
static_assert(!ldpc::bs::Geo<ldpc::EMU_CODE>::TWO_WAVES, "the soft form exists for the one-wave codes");
// the soft decoder: app [batch][n + p] i8 beside the three hard results.  1: an LDS, alignment or global-bounds fault of the kernel text
extern "C" int bsa_emu_decode(const int8_t *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run<ldpc::EMU_CODE, true>(llrs, app, out, iters, ok, batch, maxiters); });
}
// the plain decoder (SOFT = false) from the same header text
extern "C" int bsa_emu_decode_plain(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run<ldpc::EMU_CODE, false>(llrs, nullptr, out, iters, ok, batch, maxiters); });
}
extern "C" int bsa_emu_group(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::G; }
extern "C" int bsa_emu_code(void) { return ldpc::EMU_CODE; }
extern "C" int bsa_emu_planes_in_lds(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::SOFT_LDS ? 1 : 0; }
extern "C" int bsa_emu_lds_bytes(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::LDS_BYTES_SOFT; }
extern "C" int bsa_emu_plain_lds_bytes(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::LDS_BYTES; }
