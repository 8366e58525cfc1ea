"""Torch restatement of the semantic cross-entropy that include/sgr_semantic_loss.h declares: the oracle of
tests/test_semantic_loss_cpu.py and tests/test_gpu_semantic_loss.py in float64, and -- the same text in float32 -- the
yardstick their floating-point bounds are taken from and the "torch formulation" tools/bench_semantic_loss.py times.
Gradients come from autograd.  Also the seeded inputs the two test files share."""
import torch
import torch.nn.functional as F

NAMES = ("loss", "n_valid", "n_out_of_range", "accuracy")
EPS = 1e-8
_IGNORE = -100  # what every pixel that does not count is mapped to before F.cross_entropy / F.nll_loss


def classify(labels, S, ignore_index):
    """-> (valid, out_of_range) boolean maps: valid = in [0, S) and not ignore_index; out of range = >= S and not ignore_index."""
    lab = labels.reshape(labels.shape[-2:]).to(torch.int64)
    keep = lab != ignore_index
    return (lab >= 0) & (lab < S) & keep, (lab >= S) & keep


def formulation(semantic, target, mode, ignore_index):
    """The loss alone, as a trainer writes it in torch, on a flat int64 `target` whose every entry is in [0, S) or is
    `ignore_index`.  logits: F.cross_entropy on the [H*W, S] view; probabilities: street_gaussian_renderer.py:261-262
    restated, then F.nll_loss."""
    S = semantic.shape[0]
    if mode == "logits":
        return F.cross_entropy(semantic.permute(1, 2, 0).reshape(-1, S), target, ignore_index=ignore_index)
    if mode == "probabilities":
        r = semantic / (torch.sum(semantic, dim=0, keepdim=True) + EPS)  # normalize to probabilities        :261
        r = torch.log(r + EPS)                                           # change for cross entropy loss     :262
        return F.nll_loss(r.permute(1, 2, 0).reshape(-1, S), target, ignore_index=ignore_index)
    raise ValueError(mode)


def semantic_loss(semantic, labels, *, mode="logits", ignore_index=-1):
    """-> dict(loss, n_valid, n_out_of_range, accuracy, pred, valid) in semantic's dtype: `formulation` with every label
    that does not count mapped to the ignored value first; accuracy and the arg-max image from argmax(dim=0)."""
    S, H, W = semantic.shape
    valid, oor = classify(labels, S, ignore_index)
    lab = labels.reshape(H, W).to(torch.int64)
    loss = formulation(semantic, torch.where(valid, lab, torch.full_like(lab, _IGNORE)).reshape(-1), mode, _IGNORE)
    pred = semantic.detach().argmax(dim=0)
    n_valid = valid.sum()
    return dict(loss=loss, n_valid=n_valid, n_out_of_range=oor.sum(), accuracy=((pred == lab) & valid).sum().double() / n_valid,
                pred=pred, valid=valid)


def loss_and_grad(semantic, labels, dtype, *, mode, ignore_index=-1, upstream=1.0):
    """The restatement in `dtype` on semantic's device -> (dict as above, d(upstream * loss)/d semantic)."""
    x = semantic.detach().to(dtype).requires_grad_(True)
    out = semantic_loss(x, labels, mode=mode, ignore_index=ignore_index)
    (out["loss"] * upstream).backward()
    return out, x.grad


def near_ties(semantic):
    """Pixels whose two largest values (in float64) differ, but by less than float32 resolves: their arg-max is not pinned."""
    if semantic.shape[0] < 2:
        return torch.zeros(semantic.shape[1:], dtype=torch.bool, device=semantic.device)
    top = semantic.detach().to(torch.float64).topk(2, dim=0).values
    gap = top[0] - top[1]
    return (gap > 0) & (gap < 2.0 ** -24 * top[0].abs())


# ---- seeded inputs -------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 5, 7), (19, 67, 131), (32, 33, 65)]


def make_semantic(mode, S, H, W, seed=0):
    """logits: normal * 8, and on 1 % of the pixels one channel at +80 and another at -80 (a kernel that does not subtract
    the maximum overflows there).  probabilities: alpha-weighted softmax rows that sum to a random coverage in [0, 1], and
    2 % of the pixels all zero (the eps paths).  float32, on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + S * 7 + H * 3 + W)
    n = H * W
    if mode == "logits":
        x = torch.randn(S, n, generator=g) * 8.0
        if S >= 2:
            pix = torch.nonzero(torch.rand(n, generator=g) < 0.01).reshape(-1)
            hi = torch.randint(0, S, (pix.numel(),), generator=g)
            lo = (hi + 1 + torch.randint(0, S - 1, (pix.numel(),), generator=g)) % S
            x[hi, pix] = 80.0
            x[lo, pix] = -80.0
    else:
        x = torch.softmax(torch.randn(S, n, generator=g) * 3.0, dim=0) * torch.rand(1, n, generator=g)
        x[:, torch.rand(n, generator=g) < 0.02] = 0.0
    return x.reshape(S, H, W).contiguous()


def make_labels(S, H, W, dtype=torch.int64, ignore_index=-1, seed=0, n_bad=5):
    """Uniform in [-1, S) (about 1 / (S + 1) of the pixels ignored), then `n_bad` labels >= S where the map has room for
    them.  -1 becomes `ignore_index` (255 for uint8)."""
    g = torch.Generator().manual_seed(2000 * seed + S * 5 + H * 11 + W)
    n = H * W
    lab = torch.randint(-1, S, (n,), generator=g)
    if n >= 8 * n_bad:
        where = torch.randperm(n, generator=g)[:n_bad]
        lab[where] = S + torch.randint(0, 3, (n_bad,), generator=g)
    lab = torch.where(lab < 0, torch.full_like(lab, ignore_index), lab)
    return lab.reshape(H, W).to(dtype)


def bounds(semantic, labels, *, mode, ignore_index=-1, upstream=1.0):
    """-> (oracle dict, oracle gradient, loss bound, gradient bound, gradient scale) on semantic's device.
    The yardstick is the deviation of torch's own float32 formulation from the float64 oracle on the same inputs; the op may
    deviate by max(4 x yardstick, 16 x 2^-24 x scale), scale = the largest |x| for the loss (lse - x_l cancels at that
    magnitude) and the largest reference element for the gradient.  The bounds are absolute."""
    o64, g64 = loss_and_grad(semantic, labels, torch.float64, mode=mode, ignore_index=ignore_index, upstream=upstream)
    o32, g32 = loss_and_grad(semantic, labels, torch.float32, mode=mode, ignore_index=ignore_index, upstream=upstream)
    floor = 16 * 2.0 ** -24
    loss_bound = max(4 * abs(o32["loss"].item() - o64["loss"].item()), floor * semantic.abs().max().item())
    gscale = g64.abs().max().item()
    grad_bound = max(4 * (g32.double() - g64).abs().max().item(), floor * gscale)
    return o64, g64, loss_bound, grad_bound, gscale
