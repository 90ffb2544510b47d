#!/usr/bin/env python3
"""Where does the row-driven item pass of a gathered minibatch beat the column-driven one?  Forward + backward of the fused ELBO (2PL,
ability_dim 8) on sparse response rows, one GPU, one process, two legs per row on the same image, the same persons and the same build:

    columns  vibo_sparse_elbo_fwd_bwd_gather on rows.take(idx)                       (the item pass streams the image's whole column side)
    rows     vibo_sparse_elbo_fwd_bwd_gather_rows on rows.take(idx, item_pass='rows') (the batch's cells as keys, sorted, summed by segment)

at 100k x 10k with densities 2 % and 0.1 % for B = 16, 1 024, 16 384 and P persons (the shapes of profiles/sparse_gather_record.txt),
and at 1M x 100k with about 32 cells per row for B = 16, 1 024 and 16 384 (a 128 MB column side and no dense format).  Timed as
tools/sparse_crossover.py times its legs (its time_blocks: warm-up, the legs alternating in --blocks blocks, device events around work
that ends in a synchronise, median (min - max) of the blocks' per-launch times).  At every timed size the two legs' outputs are compared
first (heads and per-person outputs to 2e-5, gradients to 1e-4 of the tensor's largest entry; the person pass's outputs are also held
bit for bit); a row that misses says so instead of a time.  "keys": cap = B x the image's longest row, what the row-driven leg sorts.

    python tools/sparse_row_driven.py --out profiles/sparse_row_driven_record_table.txt

A run without a GPU fails: there is no fallback and no number.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from sparse_crossover import A, IRT, draw_matrix, fmt_ms, problem, time_blocks, worst_disagreement  # noqa: E402
from vibo_amd import _lib, ops, sparse  # noqa: E402
from vibo_amd.sparse import SparseRows  # noqa: E402

SQUARE = ((100_000, 10_000), (0.02, 0.001), (16, 1_024, 16_384, None))          # shape, densities, batches (None: every person)
WIDE = ((1_000_000, 100_000), 32, (16, 1_024, 16_384))                           # shape, cells per row, batches

HEAD = (f'{"shape":>16} {"density":>8} {"cells":>12} {"B":>7} {"batch cells":>12} {"longest row":>11} {"keys":>10} | {"columns leg ms":>28} '
        f'{"rows leg ms":>28} {"rows / columns":>14} | {"column side MB":>14} | rows agrees with columns')


def measure(rows, label, density, batches, table, item, eps, spec, gen, args):
    P, I = rows.image_persons, rows.num_item
    lines = []
    for B in batches:
        B = P if B is None else min(B, P)
        idx = torch.randperm(P, device=rows.device, generator=gen)[:B].contiguous()
        by_columns, by_rows, e = rows.take(idx), rows.take(idx, item_pass='rows'), eps[:B].contiguous()

        def columns_leg():
            return sparse._hip_sparse_elbo(spec, by_columns, table, item, e, _lib.REG_KL, True)

        def rows_leg():
            return sparse._hip_sparse_elbo(spec, by_rows, table, item, e, _lib.REG_KL, True)

        r, c = rows_leg(), columns_leg()
        ok, why = worst_disagreement(r, c, (I, spec.item_dim))
        same = torch.equal(r.scalars, c.scalars) and torch.equal(r.ability, c.ability) and torch.equal(r.grad_table(0), c.grad_table(0))
        ok, why = ok and same, why + ('; person pass bit-identical' if same else '; PERSON PASS BITS DIFFER')
        del r, c
        torch.cuda.synchronize()
        t = time_blocks({'columns': columns_leg, 'rows': rows_leg}, args.blocks, args.block_seconds)
        batch_cells = int((rows.row_ptr[idx + 1] - rows.row_ptr[idx]).sum())
        ratio = statistics.median(t['rows']) / statistics.median(t['columns'])
        lines.append(f'{label:>16} {density:8.3%} {rows.nnz:12d} {B:7d} {batch_cells:12d} {rows.max_row_cells:11d} {B * rows.max_row_cells:10d} | '
                     f'{fmt_ms(t["columns"]):>28} {fmt_ms(t["rows"]) if ok else "outputs differ":>28} {ratio:14.2f} | '
                     f'{4 * rows.nnz / 1e6:14.1f} | {"yes" if ok else "NO"}: {why}')
        print(lines[-1], flush=True)
    assert rows.bad_index_count == 0 and bool((rows.slot_map() == _lib.SPARSE_NO_SLOT).all())
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per leg, alternating (at least 5)')
    ap.add_argument('--block-seconds', type=float, default=0.15, help='launches per block are sized to about this long')
    ap.add_argument('--scale', type=float, default=1.0, help='scale every person count (rehearsals; the record is taken at 1.0)')
    ap.add_argument('--skip-wide', action='store_true', help='leave out the 1M x 100k rows')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('sparse_row_driven: no GPU -- nothing is measured without one')
    if args.blocks < 5:
        raise SystemExit('sparse_row_driven: at least 5 blocks')
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    spec = ops.ElboSpec(irt_model=IRT, ability_dim=A)
    lines = ['command: python tools/sparse_row_driven.py ' + ' '.join(sys.argv[1:] if argv is None else argv),
             f'device: {torch.cuda.get_device_name(0)}; 2PL, ability_dim {A}, forward + backward, VIBO_SPARSE_CHUNK {_lib.SPARSE_CHUNK}',
             'ms per launch: median (min - max) over %d alternating blocks' % args.blocks, '', HEAD]
    print(HEAD, flush=True)

    (P0, I), densities, batches = SQUARE
    P = max(64, int(P0 * args.scale))
    table, item, eps = problem(P, I, gen, dev)
    for density in densities:
        right, observed = draw_matrix(P, I, density, gen, dev)
        rows = SparseRows._from_observed(observed, right)
        del right, observed
        lines += measure(rows, f'{P} x {I}', density, batches, table, item, eps, spec, gen, args)
        del rows
        torch.cuda.empty_cache()
    if not args.skip_wide:
        (P0, I), per_row, batches = WIDE
        P = max(64, int(P0 * args.scale))
        table, item, eps = problem(P, I, gen, dev)
        key = torch.unique(torch.arange(P, device=dev).repeat_interleave(per_row) * I + torch.randint(0, I, (P * per_row,), device=dev, generator=gen))
        rows = SparseRows.from_coo(key // I, key % I, torch.rand(key.numel(), device=dev, generator=gen) < 0.5, P, I, check=False)
        del key
        lines += measure(rows, f'{P} x {I}', rows.density, batches, table, item, eps[:max(batches)], spec, gen, args)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
