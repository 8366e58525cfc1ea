// blend_step_host.hip -- the host-compilable part of the forward blend step's weight (street_gaussians_amd/csrc/sgr_math.h:
// sgr_blend_weight), compiled for the host (hipcc -x hip --cuda-host-only) so that tests/test_blend_step_host_cpu.py runs
// the text the gfx950 kernels run.  The lane mask of the kernels (sgr_sel_mask on an SGPR pair) is a plain ?: here.
#include "../../street_gaussians_amd/csrc/sgr_math.h"

extern "C" {

// one_select[i] = sgr_blend_weight(blends ? alpha : 0, T): the form the parity-mode forward runs;
// two_selects[i] = blends ? alpha * T : 0: the form it replaced (and the one the default mode keeps).  Written to memory as
// floats; the caller compares bytes.
void bs_weights(int n, const float* alpha, const float* T, const unsigned char* blends, float* one_select, float* two_selects) {
#pragma clang fp contract(off)
    for (int i = 0; i < n; i++) {
        const float ae = blends[i] ? alpha[i] : 0.0f;
        one_select[i] = sgr_blend_weight(ae, T[i]);
        const float prod = alpha[i] * T[i];
        two_selects[i] = blends[i] ? prod : 0.0f;
    }
}

}  // extern "C"
