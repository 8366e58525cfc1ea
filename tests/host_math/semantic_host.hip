// semantic_host.hip -- the per-pixel arithmetic of the semantic cross-entropy (street_gaussians_amd/csrc/sgr_semantic.h),
// compiled for the host (hipcc -x hip --cuda-host-only) so that tests/test_semantic_loss_cpu.py runs the text the gfx950
// kernels run: a loop over the pixels where the kernels have a lane each.
#include "../../street_gaussians_amd/csrc/sgr_semantic.h"

template <int NC>
static void forward_nc(int S, size_t plane, const float* sem, const void* labels, int dtype, int ignore_index, int mode,
                       float* loss_p, uint8_t* pred, uint8_t* cls) {
    for (size_t p = 0; p < plane; p++) {
        const int64_t lab = sem_label(labels, dtype, p);
        cls[p] = (uint8_t)sem_classify(lab, S, ignore_index);
        float x[NC], loss;
        int best;
        sem_load<NC>(x, sem, plane, p, S);
        sem_forward_point<NC>(x, S, mode, cls[p] == SGR_SEM_PIX_VALID ? (int)lab : -1, loss, best);
        loss_p[p] = cls[p] == SGR_SEM_PIX_VALID ? loss : 0.f;
        pred[p] = (uint8_t)best;
    }
}

template <int NC>
static void backward_nc(int S, size_t plane, const float* sem, const void* labels, int dtype, int ignore_index, int mode,
                        float scale, float* grad) {
    for (size_t p = 0; p < plane; p++) {
        const int64_t lab = sem_label(labels, dtype, p);
        float x[NC] = {};
        if (sem_classify(lab, S, ignore_index) == SGR_SEM_PIX_VALID) {
            sem_load<NC>(x, sem, plane, p, S);
            sem_backward_point<NC>(x, S, mode, (int)lab, scale);
        }
        for (int c = 0; c < S; c++) grad[c * plane + p] = x[c];
    }
}

extern "C" {

// loss_p [plane] (0 on pixels that do not count), pred [plane] the first-maximum channel, cls [plane] 0 ignored / 1 valid /
// 2 out of range
void sh_forward(int S, int H, int W, const float* sem, const void* labels, int dtype, int ignore_index, int mode, float* loss_p,
                uint8_t* pred, uint8_t* cls) {
    const size_t plane = (size_t)H * W;
    if (S <= 8) forward_nc<8>(S, plane, sem, labels, dtype, ignore_index, mode, loss_p, pred, cls);
    else if (S <= 16) forward_nc<16>(S, plane, sem, labels, dtype, ignore_index, mode, loss_p, pred, cls);
    else if (S <= 24) forward_nc<24>(S, plane, sem, labels, dtype, ignore_index, mode, loss_p, pred, cls);
    else forward_nc<32>(S, plane, sem, labels, dtype, ignore_index, mode, loss_p, pred, cls);
}

// grad [S][plane] <- scale * d loss_p / d x_c on valid pixels, 0 elsewhere
void sh_backward(int S, int H, int W, const float* sem, const void* labels, int dtype, int ignore_index, int mode, float scale,
                 float* grad) {
    const size_t plane = (size_t)H * W;
    if (S <= 8) backward_nc<8>(S, plane, sem, labels, dtype, ignore_index, mode, scale, grad);
    else if (S <= 16) backward_nc<16>(S, plane, sem, labels, dtype, ignore_index, mode, scale, grad);
    else if (S <= 24) backward_nc<24>(S, plane, sem, labels, dtype, ignore_index, mode, scale, grad);
    else backward_nc<32>(S, plane, sem, labels, dtype, ignore_index, mode, scale, grad);
}

}  // extern "C"
