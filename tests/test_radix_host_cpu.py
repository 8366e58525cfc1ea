"""The digit-counts-to-first-slots step of the radix kernels (street_gaussians_amd/csrc/sgr_radix.h: sgr_bin_counts,
sgr_bin_starts), compiled for the host and run owner by owner by tests/host_math/host_math.hip (hm_bin_starts; the scan of
the owners' sums between the two halves is the harness's), against numpy: start[w][d] = the counts of every digit below d in
all waves + the counts of digit d in the waves below w.  Integers: equality is exact.  The configurations are the ones the
kernels instantiate -- the scatter of sgr_scan_sort.hip (lane l of wave 0 owns the bins from l * bins / 64 on, 5- to 9-bit
digits; at 32 bins half the lanes idle) and its one-sweep form (thread d owns bin d), and the per-tile sorts of
sgr_tile_sort.hip (one wave: 8 bins per lane; 8 and 16 waves: one bin per thread, at 16 waves half the threads idle).
No GPU needed."""
import numpy as np
import pytest

from test_host_math import _p, hm  # noqa: F401  (hm: the module-scoped fixture that builds and loads the host library)

# (site, waves, bins, owners, bins per owner)
CONFIGS = [("scatter", 4, 32, 64, 1), ("scatter", 4, 64, 64, 1), ("scatter", 4, 128, 64, 2), ("scatter", 4, 256, 64, 4),
           ("scatter", 4, 512, 64, 8), ("scatter_one_sweep", 4, 256, 256, 1), ("tile_sort_wave", 1, 512, 64, 8),
           ("tile_sort_block", 8, 512, 512, 1), ("tile_sort_block", 16, 512, 1024, 1)]


def _counts(kind, waves, bins, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":  # many empty (wave, digit) cells, a few heavy ones
        c = rng.integers(0, 70, (waves, bins)) * (rng.random((waves, bins)) < 0.3)
        c[rng.integers(0, waves), rng.integers(0, bins)] += 4000
    elif kind == "one_digit":  # every key of the block on one digit: 4096 keys split over the waves
        c = np.zeros((waves, bins), np.int64)
        c[:, bins - 3] = 4096 // waves
    else:  # "empty": no keys at all
        c = np.zeros((waves, bins), np.int64)
    return np.ascontiguousarray(c, dtype=np.uint32)


@pytest.mark.parametrize("kind", ["random", "one_digit", "empty"])
@pytest.mark.parametrize("site,waves,bins,owners,bpo", CONFIGS)
def test_bin_starts_match_numpy(hm, site, waves, bins, owners, bpo, kind):
    assert owners * bpo >= bins
    cnt = _counts(kind, waves, bins, seed=waves * 1000 + bins + bpo)
    per_digit = cnt.astype(np.int64).sum(axis=0)
    below = np.concatenate([[0], np.cumsum(per_digit)[:-1]])                                  # every digit below d, all waves
    in_digit = np.concatenate([np.zeros((1, bins), np.int64), np.cumsum(cnt.astype(np.int64), axis=0)[:-1]])  # digit d, waves below w
    want = (below[None, :] + in_digit).astype(np.uint32)
    got = cnt.copy()
    first = np.zeros(bins, np.uint32)
    assert hm.hm_bin_starts(waves, bins, owners, bpo, _p(got), _p(first)) == 1, "not a configuration the harness knows"
    assert np.array_equal(got, want), (site, kind, int((got != want).sum()))
    assert np.array_equal(first, want[0]), (site, kind)  # the per-bin hook saw every bin once, with the bin's first slot
