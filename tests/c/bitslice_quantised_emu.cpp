// CPU emulation of the bit-sliced i8 decoder READING F32 LLRs (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp,
// load_column_planes<..., QuantisedF32>, plain and Decoder<..., CORRECTED = true, MULBITS>): the SAME source text the
// gfx950 kernels of decode_ms_bs_quantised.hip are compiled from, instantiated with the emulators' 64-lane, address-checked backend
// (tests/c/bitslice_emu_backend.hpp) and the f32 loader's quantiser added to it -- the library's own (ldpc::quantise_llr of
// llr_quantise.hpp, compiled here by g++ for the host).  Test infrastructure (tests/test_bitslice_quantised_emu.py compares it with the
// restatements on the CPU); it is not part of the product.
//   g++ -O1 -std=c++20 -fno-fast-math -ffp-contract=off -shared -fPIC -DEMU_CODE=TM8192 -D__HIP_PLATFORM_AMD__ -I<rocm>/include
//       -Ilabrador_ldpc_amd/csrc tests/c/bitslice_quantised_emu.cpp -o build/libbitslice_quantised_emu_TM8192.so
#define BS_FN inline
#include "decode_ms_bitslice.hpp"
#include "llr_quantise.hpp"

#include "bitslice_emu_backend.hpp"

namespace {

// the backend with the f32 loader's quantiser: four f32 LLRs (their bits) -> one dword of four i8 bytes by the library's one rule
struct F32Backend : EmuBackend {
    using EmuBackend::EmuBackend;
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
};

// the one-wave lockstep driver, group after group (decode_ms_bsq_kernel<CODE>, decode_ms_bsqc_kernel<CODE, MULBITS>): the LDS store
// has exactly the layout's size, so an address beyond it throws here
template <int CODE, bool CORRECTED, int MULBITS, class SRC>
int run(const typename SRC::T *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, uint32_t scale_num,
        uint32_t scale_shift, uint32_t offset, SRC source)
{
    using GEO = ldpc::bs::Geo<CODE>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        F32Backend b(GEO::LDS_BYTES);
        ldpc::bs::init_kernel<CODE, F32Backend>(b);
        ldpc::bs::decode_group<CODE, F32Backend, CORRECTED, MULBITS, false, SRC>(b, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g,
                                                                                 scale_num, scale_shift, offset, nullptr, source);
    }
    return 0;
}

}  // namespace

// One code per shared object (-DEMU_CODE=TM8192 ...): the instantiations compile in parallel (tests/test_bitslice_quantised_emu.py).
#ifndef EMU_CODE
#error "compile with -DEMU_CODE=<TM1536|TM2048|TM6144|TM8192>"
#endif
static_assert(ldpc::bs::bitsliced_soft_code(ldpc::EMU_CODE), "the f32 loader exists for the one-wave codes");
extern "C" int bsq_emu_mulbits(uint32_t scale_num, uint32_t scale_shift) { return ldpc::bs::correction_mulbits(scale_num, scale_shift); }
// The decoder on f32 rows at (scale, lim).  mulbits < 0: the plain form (decode_ms_bsq_kernel); else the corrected form built for
// `mulbits` multiplier bits (0, 4, 8; the triple must fit the form).  1: an LDS, alignment or global-bounds fault of the kernel text;
// 2: no such form, or the triple does not fit it
extern "C" int bsq_emu_decode(const float *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, float scale,
                              float lim, uint32_t scale_num, uint32_t scale_shift, uint32_t offset, int mulbits)
{
    using ldpc::bs::QuantisedF32;
    if (mulbits >= 0 && (scale_shift > 8 || ldpc::bs::correction_mulbits(scale_num, scale_shift) > mulbits)) return 2;
    const QuantisedF32 src{scale, lim};
    return faults_to_1([&] {
        switch (mulbits) {
            case -1: return run<ldpc::EMU_CODE, false, 8, QuantisedF32>(llrs, out, iters, ok, batch, maxiters, 1, 0, 0, src);
            case 0: return run<ldpc::EMU_CODE, true, 0, QuantisedF32>(llrs, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, src);
            case 4: return run<ldpc::EMU_CODE, true, 4, QuantisedF32>(llrs, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, src);
            case 8: return run<ldpc::EMU_CODE, true, 8, QuantisedF32>(llrs, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, src);
            default: return 2;
        }
    });
}
// the i8-source decoder of the same header, plain form (decode_ms_bs_kernel's lockstep text): the default SRC
extern "C" int bsq_emu_decode_i8(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run<ldpc::EMU_CODE, false, 8, ldpc::bs::RawI8>(llrs, out, iters, ok, batch, maxiters, 1, 0, 0, {}); });
}
// the library's quantiser as this build compiled it
extern "C" void bsq_emu_quantise(const float *x, int8_t *q, size_t count, float scale, float lim)
{
    for (size_t i = 0; i < count; ++i) q[i] = ldpc::quantise_llr<int8_t>(x[i], scale, lim);
}
extern "C" int bsq_emu_group(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::G; }
extern "C" int bsq_emu_code(void) { return ldpc::EMU_CODE; }
extern "C" int bsq_emu_lds_bytes(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::LDS_BYTES; }
