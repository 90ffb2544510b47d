"""The matrix kernel's paired code words on tile rows (csrc/vibo_msplit_kernel.hpp, pair_words; vibo_variant.hpp, ms_word_pairs), one byte
position at a time.

On tile rows the kernel interleaves the bytes of neighbouring code words in registers -- once in the prologue, once per batch in the loop --
and every tile converts two bytes of the result.  A wrong selector byte sends one class of cells to another tile or person; the random
matrices of test_gpu_tile_rows.py would notice that but not name it.  Here each of 64 matrices is observed (and answered right) in ONE
class of cells and missing everywhere else: rows p with p % 4 == j and (p // 16) % 2 == h, items i with i % 4 == t and (i // 64) % 2 == u
-- one byte position of one word of a lane.  The reference is the same library's launch on the source rows, every output bit for bit."""
import functools
import itertools

import pytest
import torch

from gpu_common import dev
from tile_rows_gpu_common import assert_same_outputs, both, build, grid_of, problem
from vibo_amd import _lib

pytestmark = pytest.mark.gpu

CLASSES = list(itertools.product(range(4), range(2), range(4), range(2)))        # (j, h, t, u)
# 1000 items: 8 waves, the one-barrier loop; 500: 4 waves, the two-barrier loop (ms_word_pairs covers every tile-rows instantiation)
WIDTHS = [1000, 500]


def persons(I):
    """One batch more than the launch has workgroups, and 7 rows: workgroup 0 pairs the words of its first batch in the prologue and
    those of its second at the loop's back edge, and the last batch is partial."""
    return 32 * (grid_of(I) + 1) + 7


@functools.lru_cache(maxsize=2)
def shared(I):
    """(spec, table, item sample, row numbers, item numbers) of a width, made once and never written."""
    return problem(2, 8, I) + (torch.arange(persons(I), device=dev()), torch.arange(I, device=dev()))


@pytest.mark.parametrize('I', WIDTHS, ids=lambda I: f'{I} items')
@pytest.mark.parametrize('j,h,t,u', CLASSES, ids=[f'row {j} of 4, half {h} | item {t} of 4, u-step {u}' for j, h, t, u in CLASSES])
def test_one_class_of_cells(j, h, t, u, I):
    spec, table, item, p, i = shared(I)
    rows = (p % 4 == j) & ((p // 16) % 2 == h)
    cols = (i % 4 == t) & ((i // 64) % 2 == u)
    m = (rows[:, None] & cols[None, :]).to(torch.uint8)
    r = m.float()                                      # observed cells answered right, 0.0 under the mask
    n_obs = int(rows.sum()) * int(cols.sum())
    assert n_obs > 0
    image = build(r, m, _lib.MASK_U8, r.shape[0])
    ref, got = both(spec, r, m, _lib.MASK_U8, image, table, item)
    assert_same_outputs(ref, got, n_obs)
