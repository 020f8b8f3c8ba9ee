// CPU emulation of the bit-sliced i8 decoder WITH normalized / offset check messages (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp,
// Decoder<..., CORRECTED = true>): the SAME source text the gfx950 kernels of decode_ms_bs_corrected.hip are compiled
// from, instantiated with the emulators' 64-lane, address-checked backend (tests/c/bitslice_emu_backend.hpp).  Test infrastructure
// (tests/test_bitslice_corrected_emu.py compares it with tests/flooding_fixed_corrected_restatement.py on the CPU); it is not part of
// the product.
//   g++ -O1 -std=c++20 -shared -fPIC -DEMU_CODE=TM8192 -Ilabrador_ldpc_amd/csrc tests/c/bitslice_corrected_emu.cpp -o build/libbitslice_corrected_emu_TM8192.so
#define BS_FN inline
#include "decode_ms_bitslice.hpp"
#include "decode_ms_bitslice_split.hpp"

#include "bitslice_emu_backend.hpp"

namespace {

// the one-wave lockstep driver, group after group (decode_ms_bsc_kernel)
template <int CODE, int MULBITS>
int run(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, uint32_t num, uint32_t shift, uint32_t offset)
{
    using GEO = ldpc::bs::Geo<CODE>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        EmuBackend b(GEO::LDS_BYTES);
        ldpc::bs::init_kernel<CODE, EmuBackend>(b);
        ldpc::bs::decode_group<CODE, EmuBackend, true, MULBITS>(b, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g, num, shift, offset);
    }
    return 0;
}

// the two-waves-per-group driver (decode_ms_bsc_split_kernel): the two halves of a group run stage by stage, alternately, on one shared
// LDS store -- the order the workgroup barriers enforce on the GPU
template <int CODE, int MULBITS>
int run_split(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, uint32_t num, uint32_t shift, uint32_t offset)
{
    using namespace ldpc::bs;
    using LAY = SplitLayout<CODE>;
    using GEO = Geo<CODE, 0>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        auto store = std::make_shared<std::vector<uint8_t>>(LAY::BYTES, 0xA5);
        EmuBackend b0(store, LAY::PRIV0), b1(store, LAY::PRIV1);
        SplitGroup<CODE, EmuBackend, 0, true, MULBITS> w0;
        SplitGroup<CODE, EmuBackend, 1, true, MULBITS> w1;
        w0.init(b0); w1.init(b1);
        w0.set_correction(num, shift, offset); w1.set_correction(num, shift, offset);
        w0.prologue(b0, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g);
        w1.prologue(b1, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g);
        for (uint32_t it = 0; it < maxiters && w0.running(); ++it) {
            if (w0.running() != w1.running()) return 2;                  // the two waves must agree on every verdict
            w0.stage_columns(b0); w1.stage_columns(b1);
            w0.stage_publish(b0); w1.stage_publish(b1);
            w0.stage_merge(b0); w1.stage_merge(b1);
            w0.stage_fetch(b0); w1.stage_fetch(b1);
            w0.stage_finish(b0, it); w1.stage_finish(b1, it);
            if (w0.frozen_mask != w1.frozen_mask) return 3;
        }
        w0.epilogue(b0); w1.epilogue(b1);
    }
    return 0;
}

template <int CODE, int MULBITS>
int run_form(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, uint32_t num, uint32_t shift, uint32_t offset)
{
    // (the rate-4/5 codes exist only in the two-waves-per-group form)
    if constexpr (ldpc::bs::Geo<CODE>::TWO_WAVES) return run_split<CODE, MULBITS>(llrs, out, iters, ok, batch, maxiters, num, shift, offset);
    else return run<CODE, MULBITS>(llrs, out, iters, ok, batch, maxiters, num, shift, offset);
}

// the plane arithmetic alone: `count` <= 2048 magnitudes, value i in bit i % 32 of lane i / 32, through Decoder::correct_mag
template <int MULBITS>
void correct_planes(const uint8_t *m_in, uint8_t *m_out, size_t count, uint32_t num, uint32_t shift, uint32_t offset)
{
    using D = ldpc::bs::Decoder<ldpc::EMU_CODE, EmuBackend, -1, true, MULBITS>;
    Vec m[ldpc::bs::MG];
    for (auto &pl : m) std::memset(pl.l, 0, sizeof pl.l);
    for (size_t i = 0; i < count; ++i)
        for (int k = 0; k < ldpc::bs::MG; ++k) m[k].l[i / 32] |= (uint32_t)((m_in[i] >> k) & 1) << (i % 32);
    D::correct_mag(m, num, shift, offset);
    for (size_t i = 0; i < count; ++i) {
        uint8_t v = 0;
        for (int k = 0; k < ldpc::bs::MG; ++k) v |= (uint8_t)(((m[k].l[i / 32] >> (i % 32)) & 1) << k);
        m_out[i] = v;
    }
}

}  // namespace

// One code per shared object (-DEMU_CODE=TM8192 ...): the six instantiations compile in parallel (tests/test_bitslice_corrected_emu.py).
#ifndef EMU_CODE
#error "compile with -DEMU_CODE=<TM1280|TM1536|TM2048|TM5120|TM6144|TM8192>"
#endif
// the form the launcher takes for the triple (ldpc::bs::correction_mulbits), as launch_decode_ms_bitsliced_corrected picks it.
// 1: an LDS, alignment or global-bounds fault of the kernel text; 2 / 3: the two waves of a split group disagree
extern "C" int bsc_emu_decode(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters, uint32_t num,
                              uint32_t shift, uint32_t offset)
{
    return faults_to_1([&] {
        switch (ldpc::bs::correction_mulbits(num, shift)) {
            case 0: return run_form<ldpc::EMU_CODE, 0>(llrs, out, iters, ok, batch, maxiters, num, shift, offset);
            case 4: return run_form<ldpc::EMU_CODE, 4>(llrs, out, iters, ok, batch, maxiters, num, shift, offset);
            default: return run_form<ldpc::EMU_CODE, 8>(llrs, out, iters, ok, batch, maxiters, num, shift, offset);
        }
    });
}
// mulbits < 0: the launcher's form; else that form, which must be wide enough for the scale (-1 if it is not)
extern "C" int bsc_emu_correct(const uint8_t *m_in, uint8_t *m_out, size_t count, uint32_t num, uint32_t shift, uint32_t offset, int mulbits)
{
    const int need = ldpc::bs::correction_mulbits(num, shift);
    if (mulbits < 0) mulbits = need;
    if (count > 2048 || mulbits < need || (need == 0 && mulbits != 0)) return -1;
    switch (mulbits) {
        case 0: correct_planes<0>(m_in, m_out, count, num, shift, offset); return 0;
        case 4: correct_planes<4>(m_in, m_out, count, num, shift, offset); return 0;
        case 8: correct_planes<8>(m_in, m_out, count, num, shift, offset); return 0;
        default: return -1;
    }
}
extern "C" int bsc_emu_group(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::G; }
extern "C" int bsc_emu_code(void) { return ldpc::EMU_CODE; }
extern "C" int bsc_emu_two_waves(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::TWO_WAVES ? 1 : 0; }
