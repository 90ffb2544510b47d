"""The one-barrier batch loop of the matrix kernel on tile rows (8 waves: 897..1024 items; csrc/vibo_msplit_kernel.hpp, `OB`) at the
shapes where a pipeline two batches deep can go wrong: workgroups with 1, 2, 3, 4 and 5 batches, both parities at the tail, a partial
last batch, and launches in which some workgroups have no batch at all.

The comparison is the one of test_gpu_tile_rows.py: every output of the launch on the image against the launch on the source rows --
which runs the two-barrier loop, and which the fp64-oracle suites hold -- with torch.equal.  Every image is launched twice and the two
launches must agree bit for bit as well: a race between the waves that run a batch ahead and the waves in the tiles would show there."""
import functools

import pytest
import torch

from gpu_common import dev
from tile_rows_gpu_common import assert_same_outputs, both, build, grid_of, host_rows, problem, strided
from vibo_amd import _lib

pytestmark = pytest.mark.gpu

# batches n in units of the launch's workgroup count G: n = a G + b
BATCHES = {'1': (0, 1), 'G-1': (1, -1), 'G': (1, 0), 'G+1': (1, 1), '2G': (2, 0), '2G+1': (2, 1), '3G+1': (3, 1), '4G+3': (4, 3)}
ITEMS = (1000, 897)
TAILS = (0, 7)


def persons(I, key, tail):
    a, b = BATCHES[key]
    return 32 * (a * grid_of(I) + b) + tail


@functools.lru_cache(maxsize=2)
def all_rows(I):
    """Host rows of the largest shape at this width, made once; every case takes its first P rows (row 0 all missing, row 1 all
    observed, one item column all missing: host_rows)."""
    return host_rows(persons(I, '4G+3', max(TAILS)), I, seed=17)


def device_case(resp, mask, I):
    r, m = strided(resp, (I + 3) & ~3, 1.0), strided(mask.to(torch.uint8), (I + 3) & ~3, 1)
    return r, m, build(r, m, _lib.MASK_U8, r.shape[0]), int(mask.sum())


def same_outputs(ref, got, n_obs, I, **form):
    """assert_same_outputs, with the observed-cell count held as far as its fp32 sum can hold it: exact below 2^24 (there the count goes
    through unchanged); above, the launch on the rows may differ from the true count by the rounding of its sum over the workgroups'
    records -- one per workgroup, each exact, half an ulp of the total per addition at most -- and the launch on the image must
    still have the rows' bits."""
    seen = int(ref.scalars[_lib.S_NOBS])
    if n_obs >= 1 << 24:
        ulp = 2.0 ** (n_obs.bit_length() - 24)
        assert abs(seen - n_obs) <= grid_of(I) * ulp / 2, (seen, n_obs)
        n_obs = seen
    assert_same_outputs(ref, got, n_obs, **form)


def every_form_twice(r, m, image, n_obs, I):
    """IRT 1 / 2 / 3 at ability_dim 1 and 8: gradients with given noise, forward only, the drawing step; each on the rows and on the
    image, the image twice."""
    for irt in (1, 2, 3):
        for A in (1, 8):
            spec, table, item = problem(irt, A, I)
            for want_grad, draw in ((True, False), (False, False), (True, True)):
                ref, got = both(spec, r, m, _lib.MASK_U8, image, table, item, want_grad=want_grad, draw=draw)
                same_outputs(ref, got, n_obs, I, want_grad=want_grad, draw=draw)
                _, again = both(spec, r, m, _lib.MASK_U8, image, table, item, want_grad=want_grad, draw=draw)
                same_outputs(got, again, n_obs, I, want_grad=want_grad, draw=draw)


@pytest.mark.parametrize('tail', TAILS)
@pytest.mark.parametrize('batches', list(BATCHES))
@pytest.mark.parametrize('I', ITEMS)
def test_image_launch_equals_row_launch_and_itself(I, batches, tail):
    P = persons(I, batches, tail)
    resp, mask = all_rows(I)
    r, m, image, n_obs = device_case(resp[:P], mask[:P], I)
    every_form_twice(r, m, image, n_obs, I)


def test_count_extremes_two_batches_ahead():
    """Rows without a single answer and rows with every answer in the batches whose counts are requested from the loop, two batches
    ahead -- the third and fourth batch of workgroup 0 -- and in the partial last batch."""
    I = 1000
    G = grid_of(I)
    P = persons(I, '3G+1', 7)
    resp, mask = (t.clone() for t in all_rows(I))
    resp, mask = resp[:P], mask[:P]
    for first in (32 * 2 * G, 32 * 3 * G, P - 2):
        mask[first], mask[first + 1] = False, True
        resp[first + 1] = (resp[first + 1] == 1.0).float()      # (answers where junk lay under the mask)
    r, m, image, n_obs = device_case(resp, mask, I)
    every_form_twice(r, m, image, n_obs, I)
