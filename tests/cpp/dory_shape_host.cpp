// The round shapes of DoryCommitmentScheme.open as the device session computes them (zolt_amd/csrc/dory_shape.h), printed for every
// nu <= sigma <= 20: one line "nu sigma round cur n2 row h" per round. tests/test_dory_open_key_model.py compiles this for the host
// with -fsanitize=address,undefined and compares the lines with the reference's own loop restated in Python.
#include <stdio.h>

#include "../../zolt_amd/csrc/dory_shape.h"

int main() {
    for (uint32_t sigma = 0; sigma <= 20; sigma++)
        for (uint32_t nu = 0; nu <= sigma; nu++)
            for (uint32_t t = 0; t < sigma; t++) {
                const DoryRoundShape s = dory_round_shape(nu, sigma, t);
                printf("%u %u %u %u %u %u %u\n", nu, sigma, t, s.cur, s.n2, s.row, s.h);
            }
    return 0;
}
