/* soft_smoke.c -- a C client of the soft-output entry point (labrador_ldpc_decode_ms_soft_batch_f32): for every code, the
 * reference's test_decode_ms frame (src/decoder.rs:671-699: the codeword of data bytes 0, 1, 2, ..., three bits of byte 0
 * flipped, +-1 LLRs) decoded with 50 iterations from host buffers.  Checks success and that the sign of every transmitted
 * variable's a-posteriori LLR is the codeword's bit.  Exit status 0 = ok, 77 = no GPU, 1 = failure. */
#include "labrador_ldpc_hip.h"

#include <stdio.h>
#include <stdlib.h>

int main(void)
{
    if (labrador_ldpc_hip_device_count() == 0) {
        printf("no gfx950 device\n");
        return 77;
    }
    for (int c = LABRADOR_LDPC_CODE_TC128; c <= LABRADOR_LDPC_CODE_TM8192; c++) {
        const enum labrador_ldpc_code code = (enum labrador_ldpc_code)c;
        const size_t n = labrador_ldpc_code_n(code), k = labrador_ldpc_code_k(code);
        const size_t np = labrador_ldpc_bf_working_len(code), out_len = labrador_ldpc_output_len(code);
        uint8_t *data = malloc(k / 8), *cw = malloc(n / 8), *rx = malloc(n / 8), *out = malloc(out_len);
        float *llrs = malloc(n * sizeof(float)), *app = malloc(np * sizeof(float));
        uint32_t iters = 0;
        uint8_t success = 0;
        if (!data || !cw || !rx || !out || !llrs || !app) return 1;
        for (size_t i = 0; i < k / 8; i++) data[i] = (uint8_t)i;
        labrador_ldpc_copy_encode(code, data, cw);
        for (size_t i = 0; i < n / 8; i++) rx[i] = cw[i];
        rx[0] ^= 0xA8;
        labrador_ldpc_hard_to_llrs_f32(code, rx, llrs);
        const int st = labrador_ldpc_decode_ms_soft_batch_f32(code, llrs, app, out, &iters, &success, 1, 50, NULL);
        if (st != LABRADOR_LDPC_HIP_OK) {
            printf("code %d: status %d: %s\n", c, st, labrador_ldpc_hip_last_error());
            return 1;
        }
        if (!success) {
            printf("code %d: did not converge\n", c);
            return 1;
        }
        for (size_t j = 0; j < n; j++) {
            const int bit = (cw[j / 8] >> (7 - j % 8)) & 1, outbit = (out[j / 8] >> (7 - j % 8)) & 1;
            if ((app[j] < 0.0f) != bit || outbit != bit) {
                printf("code %d: variable %zu: app %g, codeword bit %d, output bit %d\n", c, j, (double)app[j], bit, outbit);
                return 1;
            }
        }
        printf("code %d: ok after %u iterations\n", c, iters);
        free(data); free(cw); free(rx); free(out); free(llrs); free(app);
    }
    printf("soft smoke ok\n");
    return 0;
}
