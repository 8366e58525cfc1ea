"""Scene and pins of tests/test_gpu_strict_loops.py.

tests/golden/strict_loops/pins.npz holds what the library's parity-mode forward produced for the test's calls on an MI355X
at the commit BEFORE the per-visit trims of the strict blend loops: colour, depth, alpha, the semantic image, n_contrib and
the hit record (one byte per list position, bit q = quadrant q blended it; positions behind what a tile processed are
undefined and stored as zero), per image size, mode (exact / strict) and channel count.  The trims promise every output bit,
so the test compares bytes.  Written by running this file from a checkout of that commit on the GPU:

    python tests/golden/make_strict_loops_fixture.py [output directory]

It also prints whether the backward of that commit gives the same bytes under a black and a (-0.0, 0, 0) background
(the test asserts it of the current code).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "strict_loops", "pins.npz")
SIZES = [(48, 32), (44, 30)]
CHANNELS = (0, 5)
MODES = ("strict", "exact")
FORWARD_BG = (0.3, 0.0, 0.7)


def scene(size, S):
    """300 Gaussians over six tiles, every second one nearly opaque: most pixels run into the T < 1e-4 stop, some stay open."""
    from helpers import small_case
    W, H = size
    cam, sc = small_case(P=300, W=W, H=H, S=S, seed=5, zmax=8.0, scale_px=0.05)
    sc.opacities[::2] = 0.9
    return cam, sc


def key(size, mode, S, name):
    return f"{size[0]}x{size[1]}_{mode}_S{S}_{name}"


def forward_arrays(cam, sc):
    """The forward under the caller's switch mask -> {name: numpy array}, the hit record zeroed where it is undefined."""
    from gpu_utils import npy, raw_forward, tile_tops
    from helpers import oracle_kwargs
    H, W = cam.image_height, cam.image_width
    res, internal = raw_forward(oracle_kwargs(cam, sc, bg=torch.tensor(FORWARD_BG)))
    torch.cuda.synchronize()
    out = {k: npy(res[k]).copy() for k in ("color", "depth", "alpha")}
    if sc.semantics.shape[1]:
        out["semantic"] = npy(res["semantic"]).copy()
    nc = npy(internal("n_contrib")).view(np.uint32).reshape(H, W).copy()
    ranges = npy(internal("ranges")).view(np.uint32).reshape(-1, 2).astype(np.int64)
    hits = npy(internal("hits")).reshape(-1).copy()
    n = ranges[:, 1] - ranges[:, 0]
    assert int(n.sum()) == hits.size, (int(n.sum()), hits.size)
    tile_of = np.repeat(np.arange(ranges.shape[0], dtype=np.int64), n)
    rel = np.arange(hits.size, dtype=np.int64) - ranges[tile_of, 0]
    hits[rel >= tile_tops(nc, H, W).reshape(-1)[tile_of]] = 0
    out["n_contrib"] = nc
    out["hits"] = hits
    return out


def main(outdir):
    from gpu_utils import _strict_mask, npy, raw_backward, raw_forward, switches
    from helpers import oracle_kwargs
    from street_gaussians_amd import _C
    from street_gaussians_amd import synthetic as syn
    os.makedirs(outdir, exist_ok=True)
    pins = {}
    for size in SIZES:
        for mode in MODES:
            mask = _strict_mask() if mode == "strict" else (_C.test_switches(-1) | _C.EXACT)
            for S in CHANNELS:
                cam, sc = scene(size, S)
                with switches(mask):
                    got = forward_arrays(cam, sc)
                for k, v in got.items():
                    pins[key(size, mode, S, k)] = v
            cam, sc = scene(size, 0)
            grads = []
            for bg in ((0.0, 0.0, 0.0), (-0.0, 0.0, 0.0)):
                kw = oracle_kwargs(cam, sc, bg=torch.tensor(bg))
                with switches(mask):
                    res, _ = raw_forward(kw)
                    g = raw_backward(kw, res, syn.loss_weights(cam, S=0))
                    torch.cuda.synchronize()
                grads.append({k: npy(v).copy() for k, v in g.items()})
            same = all(np.array_equal(grads[0][k].view(np.uint8), grads[1][k].view(np.uint8)) for k in grads[0])
            print(f"{size} {mode}: backward bytes under (0,0,0) and (-0.0,0,0) equal: {same}")
    path = os.path.join(outdir, "pins.npz")
    np.savez_compressed(path, **pins)
    print("wrote", path, os.path.getsize(path), "bytes,", len(pins), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(PINS))
