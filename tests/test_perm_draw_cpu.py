"""The definition of the in-engine permutation draw (`mimo_draw_permutations`), checked without a GPU on its numpy
restatement tests/perm_reference.py — the kernel is compared with that restatement bit for bit in test_perm_draw_gpu.py —
and the host side of the switch: no CPU route, documented variable."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import perm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    """The three known-answer vectors of the Random123 distribution for philox4x32-10 (kat_vectors)."""
    for ctr, key, want in (
            ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
            ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
            ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
             (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        assert tuple(int(v) for v in R.philox4x32_10(*ctr, *key)) == want


def test_keys_are_the_philox_words_with_the_index_in_the_low_bits():
    seed, offset = 0x0123456789ABCDEF, (7 << 32) | 12
    k = R.keys(3, 5, seed, offset)
    for j in range(5):
        x, y, z, w = (int(v) for v in R.philox4x32_10(j >> 1, 3, 12, 7, 0x89ABCDEF, 0x01234567))
        bits = (w << 32 | z) if j & 1 else (y << 32 | x)
        assert int(k[j]) == (bits & ~0xFFF) | j


def test_hand_checkable_cases():
    # batch = 1: the only permutation of one image, whatever the repetitions and the head count
    perm, main = R.draw_permutations(1, 3, 2, 4, seed=5, offset=0)
    assert not perm.any() and not main.any() and perm.shape == (4, 3)
    # k = 0 (input_repetition_probability = 1): every subnetwork sees the main permutation
    perm, main = R.draw_permutations(6, 1, 0, 3, seed=5, offset=4)
    assert sorted(main) == list(range(6)) and (perm == main).all()
    assert R.head_count(4, 2, 1.0) == 0 and R.head_count(7, 1, 0.9) == 0 and R.head_count(5, 3, 0.5) == 7
    # reps = 2: the main permutation tiled (torch's .repeat), the head re-shuffled per subnetwork, the tail shared
    perm, main = R.draw_permutations(5, 2, 7, 3, seed=5, offset=8)
    assert sorted(main[:5]) == list(range(5)) and (main[5:] == main[:5]).all()
    for row in perm:
        assert sorted(row[:7]) == sorted(main[:7]) and (row[7:] == main[7:]).all()
    assert len({tuple(row) for row in perm}) == 3  # three independent shuffles of 7 entries (5040 / 4 orders each)
    # another offset or seed is another draw
    assert not (R.draw_permutations(64, 1, 64, 1, 5, 0)[0] == R.draw_permutations(64, 1, 64, 1, 5, 4)[0]).all()
    assert not (R.draw_permutations(64, 1, 64, 1, 5, 0)[0] == R.draw_permutations(64, 1, 64, 1, 6, 0)[0]).all()


def _chi2_bound(df: int) -> float:
    """The chi-square quantile at 1 - 1e-6."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, df))
    except ImportError:
        a = 2.0 / (9.0 * df)  # Wilson-Hilferty at the standard normal quantile z = 4.75 (1 - 1.0e-6)
        return df * (1.0 - a + 4.75 * math.sqrt(a)) ** 3


def _chi2(counts, n):
    e = n / len(counts)
    return float(sum((c - e) ** 2 / e for c in counts))


DRAWS = 2400


def test_main_permutation_is_uniform():
    """batch = 4, S = 2, 2400 consecutive offsets from a fixed seed: the 24 orders of `main` against the uniform
    distribution.  Fixed seed = a fixed statistic: the test cannot flake."""
    index = {p: i for i, p in enumerate(itertools.permutations(range(4)))}
    counts = np.zeros(24, dtype=np.int64)
    for off in range(DRAWS):
        _, main = R.draw_permutations(4, 1, 4, 2, seed=20241008, offset=off)
        counts[index[tuple(main)]] += 1
    stat, bound = _chi2(counts, DRAWS), _chi2_bound(23)
    print(f"main, 24 cells: chi2 {stat:.1f} (bound {bound:.1f})")
    assert counts.min() > 0 and stat < bound


def test_subnetwork_shuffles_are_independent():
    """batch = 3, S = 2: the 36 joint values of (row 0, row 1) — given `main`, each row is `main` composed with its own
    uniform shuffle, so the pair is uniform on 6 x 6 exactly when the two subnetworks' draws are independent and uniform."""
    index = {p: i for i, p in enumerate(itertools.permutations(range(3)))}
    counts = np.zeros(36, dtype=np.int64)
    for off in range(DRAWS):
        perm, _ = R.draw_permutations(3, 1, 3, 2, seed=20241009, offset=off)
        counts[6 * index[tuple(perm[0])] + index[tuple(perm[1])]] += 1
    stat, bound = _chi2(counts, DRAWS), _chi2_bound(35)
    print(f"(row 0, row 1), 36 cells: chi2 {stat:.1f} (bound {bound:.1f})")
    assert counts.min() > 0 and stat < bound


@pytest.mark.parametrize("device", ["cpu", None])
def test_engine_draw_has_no_cpu_route(device):
    from mimo.models.utils import apply_input_transform
    from mimo_unet_amd._lib import MimoHipError
    from mimo_unet_amd.models.utils import draw_subnetwork_permutations
    state = torch.get_rng_state()
    with pytest.raises(MimoHipError):
        draw_subnetwork_permutations(4, 2, device=device, engine=True)
    with pytest.raises(MimoHipError):
        apply_input_transform(torch.zeros(4, 1, 8, 8), torch.zeros(4, 1, 8, 8), None, 2, engine=True)
    assert torch.equal(state, torch.get_rng_state())  # and it did not fall back to the CPU generator on the way
    assert draw_subnetwork_permutations(4, 2, device=device).shape == (2, 4)  # the default route is untouched


def test_switch_is_in_the_readme_table_and_off_by_default():
    doc = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"^\| `MIMO_ENGINE_PERM` \| 0 \|", doc, flags=re.M)
    if "MIMO_ENGINE_PERM" not in os.environ:
        from mimo_unet_amd.models import mimo_unet
        assert mimo_unet._ENGINE_PERM is False
