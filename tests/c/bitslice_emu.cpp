// CPU emulation of the bit-sliced i8 decoder (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp): the SAME source text the
// gfx950 kernel is compiled from, instantiated with a backend whose "wave register" is an array of 64 lanes and whose
// cross-lane / LDS / memory operations are plain, address-checked loops (tests/c/bitslice_emu_backend.hpp, shared by the six
// emulators).  Test infrastructure (tests/test_bitslice_emu.py compares its
// results with the oracle on the CPU, so the formulation -- layout, lane permutations, plane arithmetic, compressed row
// state -- is validated without a GPU); it is not part of the product and nothing in labrador_ldpc_amd/ links it.
//   g++ -O1 -std=c++20 -shared -fPIC -DEMU_CODE=TM8192 -Ilabrador_ldpc_amd/csrc tests/c/bitslice_emu.cpp -o build/libbitslice_emu_TM8192.so
#define BS_FN inline
#include "decode_ms_bitslice.hpp"
#include "decode_ms_bitslice_split.hpp"
#include "decode_bf_bitslice.hpp"

#include "bitslice_emu_backend.hpp"

namespace {

template <int CODE>
int run(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    using GEO = ldpc::bs::Geo<CODE>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        EmuBackend b(GEO::LDS_BYTES);
        ldpc::bs::init_kernel<CODE, EmuBackend>(b);
        ldpc::bs::decode_group<CODE, EmuBackend>(b, llrs, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g);
    }
    return 0;
}

// slot refill (decode_refill): ONE emulated wave takes the whole batch, frame after frame, a finished slot taking the next frame
template <int CODE>
int run_refill(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    using GEO = ldpc::bs::Geo<CODE>;
    if constexpr (GEO::SPLIT || GEO::G < 2 || GEO::TWO_WAVES) return -1;
    else {
        GlobalWindow window(llrs, batch, GEO::N);
        EmuBackend b(GEO::LDS_BYTES);
        ldpc::bs::init_kernel<CODE, EmuBackend>(b);
        uint32_t nextf = 0;
        ldpc::bs::decode_refill<CODE, EmuBackend>(b, llrs, out, iters, ok, maxiters,
                                                  [&]() -> uint32_t { return nextf < batch ? nextf++ : ldpc::bs::NO_FRAME; });
        return 0;
    }
}

// the two-waves-per-group kernel of the rate-4/5 codes (decode_ms_bitslice_split.hpp): the two halves of a group run stage by stage,
// alternately, on one shared LDS store -- the order the workgroup barriers enforce on the GPU
template <int CODE>
int run_split(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    using namespace ldpc::bs;
    using LAY = SplitLayout<CODE>;
    using GEO = Geo<CODE, 0>;
    GlobalWindow window(llrs, batch, GEO::N);
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    for (size_t g = 0; g < groups; ++g) {
        auto store = std::make_shared<std::vector<uint8_t>>(LAY::BYTES, 0xA5);
        EmuBackend b0(store, LAY::PRIV0), b1(store, LAY::PRIV1);
        SplitGroup<CODE, EmuBackend, 0> w0;
        SplitGroup<CODE, EmuBackend, 1> w1;
        w0.init(b0); w1.init(b1);
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

// slot refill on the two-wave kernel (decode_range_split): ONE emulated workgroup takes the whole batch as its range; the two halves
// run stage by stage on one LDS store, as run_split does
template <int CODE>
int run_split_refill(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    using namespace ldpc::bs;
    using LAY = SplitLayout<CODE>;
    GlobalWindow window(llrs, batch, Geo<CODE, 0>::N);
    auto store = std::make_shared<std::vector<uint8_t>>(LAY::BYTES, 0xA5);
    EmuBackend b0(store, LAY::PRIV0), b1(store, LAY::PRIV1);
    SplitGroup<CODE, EmuBackend, 0> w0;
    SplitGroup<CODE, EmuBackend, 1> w1;
    w0.init(b0); w1.init(b1);
    // chunks of 5 frames (not a multiple of any G): each wave walks the same sequence with a cursor of its own
    uint32_t cur0 = 0, cur1 = 0;
    auto draw_from = [&](uint32_t &cur) { return [&cur, batch]() -> uint64_t {
        if (cur >= batch) return 0;
        const uint32_t lo = cur, hi = (uint32_t)(lo + 5 < batch ? lo + 5 : batch);
        cur = hi;
        return (uint64_t)lo | (uint64_t)hi << 32; }; };
    w0.refill_begin(b0, llrs, out, iters, ok, draw_from(cur0));
    w1.refill_begin(b1, llrs, out, iters, ok, draw_from(cur1));
    for (;;) {
        w0.refill_event(b0, draw_from(cur0)); w1.refill_event(b1, draw_from(cur1));
        w0.refill_expire(b0, maxiters); w1.refill_expire(b1, maxiters);
        if (w0.rf_fin != w1.rf_fin || w0.rf_active != w1.rf_active) return 2;        // the two waves must agree on every slot
        if (w0.rf_fin) continue;
        if (!w0.rf_active) break;
        do {
            w0.d.columns(b0, ~w0.rf_active); w1.d.columns(b1, ~w1.rf_active);
            w0.stage_publish(b0); w1.stage_publish(b1);
            w0.stage_merge(b0); w1.stage_merge(b1);
            w0.stage_fetch(b0); w1.stage_fetch(b1);
            w0.refill_verdict(b0, maxiters); w1.refill_verdict(b1, maxiters);
            if (w0.rf_fin != w1.rf_fin || w0.rf_ok != w1.rf_ok) return 3;
        } while (!w0.rf_fin);
    }
    return 0;
}

// the form a code's default kernel has: the rate-4/5 codes exist only in the two-waves-per-group form
template <int CODE>
int run_default(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    if constexpr (ldpc::bs::Geo<CODE>::TWO_WAVES) return run_split<CODE>(llrs, out, iters, ok, batch, maxiters);
    else return run<CODE>(llrs, out, iters, ok, batch, maxiters);
}

// the two-wave drivers, rate 4/5 only: -1 for every other code
template <int CODE>
int run_two_waves(bool refill, const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    if constexpr (!ldpc::bs::Geo<CODE>::TWO_WAVES) return -1;
    else return refill ? run_split_refill<CODE>(llrs, out, iters, ok, batch, maxiters) : run_split<CODE>(llrs, out, iters, ok, batch, maxiters);
}

}  // namespace

// One code per shared object (-DEMU_CODE=TM8192 ...): the six instantiations compile in parallel (tests/test_bitslice_emu.py).
#ifndef EMU_CODE
#error "compile with -DEMU_CODE=<TM1280|TM1536|TM2048|TM5120|TM6144|TM8192>"
#endif
// The decode entries: 0, or 1: an LDS, alignment or global-bounds fault of the kernel text; 2 / 3: the two waves of a split group
// disagree; -1: the code has no such form
extern "C" int bs_emu_decode(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run_default<ldpc::EMU_CODE>(llrs, out, iters, ok, batch, maxiters); });
}
extern "C" int bs_emu_decode_bf(const uint8_t *input, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    // (no GlobalWindow: the bit-flipping text reads its rows with predicated gload32 alone)
    using GEO = ldpc::bs::Geo<ldpc::EMU_CODE>;
    return faults_to_1([&] {
        const size_t groups = (batch + GEO::G - 1) / GEO::G;
        for (size_t g = 0; g < groups; ++g) {
            EmuBackend b(ldpc::bs::BfGeo<ldpc::EMU_CODE>::LDS_BYTES);
            ldpc::bs::bf_init_kernel<ldpc::EMU_CODE, EmuBackend>(b);
            ldpc::bs::bf_decode_group<ldpc::EMU_CODE, EmuBackend>(b, input, out, iters, ok, (uint32_t)batch, maxiters, (uint32_t)g);
        }
        return 0;
    });
}
extern "C" int bs_emu_decode_split(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run_two_waves<ldpc::EMU_CODE>(false, llrs, out, iters, ok, batch, maxiters); });
}
extern "C" int bs_emu_decode_refill(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run_refill<ldpc::EMU_CODE>(llrs, out, iters, ok, batch, maxiters); });
}
extern "C" int bs_emu_decode_split_refill(const int8_t *llrs, uint8_t *out, uint32_t *iters, uint8_t *ok, size_t batch, uint32_t maxiters)
{
    return faults_to_1([&] { return run_two_waves<ldpc::EMU_CODE>(true, llrs, out, iters, ok, batch, maxiters); });
}
extern "C" int bs_emu_group(void) { return ldpc::bs::Geo<ldpc::EMU_CODE>::G; }
extern "C" int bs_emu_code(void) { return ldpc::EMU_CODE; }
