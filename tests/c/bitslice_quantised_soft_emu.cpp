// CPU emulation of the bit-sliced i8 decoder READING F32 LLRs WITH soft output (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp,
// decode_group<..., SOFT = true, QuantisedF32>, plain and CORRECTED = true at MULBITS 0 / 4 / 8): the SAME source text
// the gfx950 kernels of decode_ms_bs_quantised_soft.hip are compiled from -- the f32 loader, the iteration, the correction step, the kept
// planes, store_marginals -- instantiated with the emulators' 64-lane, address-checked backend (tests/c/bitslice_emu_backend.hpp): its
// LDS is bounds-checked against exactly Geo::LDS_BYTES_SOFT of the shipped placement and its 16-byte global loads must stay inside the
// batch's rows.  The f32 loader's quantiser, added here, is the library's own (ldpc::quantise_llr of llr_quantise.hpp, compiled here by
// g++ for the host).  Test infrastructure (tests/test_bitslice_quantised_soft_emu.py compares it with the restatements on the CPU); it
// is not part of the product.
//   g++ -O1 -std=c++20 -fno-fast-math -ffp-contract=off -shared -fPIC -DEMU_CODE=TM8192 -D__HIP_PLATFORM_AMD__ -I<rocm>/include
//       -Ilabrador_ldpc_amd/csrc tests/c/bitslice_quantised_soft_emu.cpp -o build/libbitslice_quantised_soft_emu_TM8192.so
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

// the one-wave lockstep driver, group after group (decode_ms_bsqa_kernel<CODE>, decode_ms_bsqca_kernel<CODE, MULBITS>): the LDS store
// has exactly the soft layout's size, so an address beyond it throws here
template <int CODE, bool CORRECTED, int MULBITS, class SRC>
int run(const typename SRC::T *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters,
        uint32_t scale_num, uint32_t scale_shift, uint32_t offset, SRC source)
{
    using GEO = ldpc::bs::Geo<CODE>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        F32Backend b(GEO::LDS_BYTES_SOFT);
        ldpc::bs::init_kernel<CODE, F32Backend>(b);
        ldpc::bs::decode_group<CODE, F32Backend, CORRECTED, MULBITS, true, SRC>(b, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g,
                                                                                scale_num, scale_shift, offset, app, source);
    }
    return 0;
}

template <class SRC>
int run_form(const typename SRC::T *llrs, int8_t *app, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters,
             uint32_t scale_num, uint32_t scale_shift, uint32_t offset, int mulbits, SRC source)
{
    if (mulbits >= 0 && (scale_shift > 8 || ldpc::bs::correction_mulbits(scale_num, scale_shift) > mulbits)) return 2;
    return faults_to_1([&] {
        switch (mulbits) {
            case -1: return run<ldpc::EMU_CODE, false, 8, SRC>(llrs, app, out, iters, ok, batch, maxiters, 1, 0, 0, source);
            case 0: return run<ldpc::EMU_CODE, true, 0, SRC>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, source);
            case 4: return run<ldpc::EMU_CODE, true, 4, SRC>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, source);
            case 8: return run<ldpc::EMU_CODE, true, 8, SRC>(llrs, app, out, iters, ok, batch, maxiters, scale_num, scale_shift, offset, source);
            default: return 2;
        }
    });
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
