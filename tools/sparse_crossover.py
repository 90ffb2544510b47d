#!/usr/bin/env python3
"""Where do sparse response rows beat the dense engine?  Forward + backward of the fused ELBO (2PL, ability_dim 8) on one GPU, in
one process, at densities 50 %, 10 %, 2 %, 0.5 % and 0.1 % of 1M x 1k and 100k x 10k, two legs per row:

    dense    cell codes (1 byte per cell of the matrix) on the kernel the planner chooses   (ops._hip_launch_elbo)
    sparse   vibo_sparse_elbo_fwd_bwd on the image of the same matrix                       (sparse._hip_sparse_elbo)

and the sparse leg alone at 1M x 100k with about 32 cells per row, where no dense format exists.  Each leg is warmed up; the legs
alternate in --blocks blocks of a few launches each, timed with device events around work that ends in a synchronise; a row
reports the median (min - max) of the blocks' per-launch times.  Before a time is quoted the two legs' outputs are compared at the
timed size: heads and per-person outputs to 2e-5, gradients to 1e-4 of the tensor's largest entry (the bounds of
tests/gpu_common.compare_raw); a row that misses them says so instead of a time.  Bytes per observed cell are counted from the
shapes: dense 1 / density (one code byte per cell of the matrix); sparse 12 streamed (row side twice, column side once, 4 bytes each)
plus the gathered 4 (D + A) (the item's row in the person pass, theta in the item pass: cache traffic while the two tables fit).

    python tools/sparse_crossover.py --out profiles/sparse_rows_record_table.txt

--gathered times minibatches instead (include/vibo_hip_sparse_gather.h): at 100k x 10k and densities 2 % and 0.1 %, forward + backward
for B = 1 024, 16 384 and P persons of the resident matrix, three legs per row:

    gather   vibo_sparse_elbo_fwd_bwd_gather on rows.take(randperm(P)[:B])                 (the item pass streams the whole column side)
    range    vibo_sparse_elbo_fwd_bwd on B consecutive persons of the same image           (the item pass bisects its chunks to the range)
    codes    the cell-code format's in-kernel gather of the same B persons (row_index)     (B x I code bytes)

timed the same way; the gather leg is compared with the codes leg on the same persons before a time is quoted.

    python tools/sparse_crossover.py --gathered --out profiles/sparse_gather_record_table.txt

A run without a GPU fails: there is no fallback and no number.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'variational-item-response-theory-public_amd'))

import torch  # noqa: E402

from vibo_amd import _lib, ops, sparse  # noqa: E402
from vibo_amd.sparse import SparseRows  # noqa: E402

A, IRT = 8, 2
DENSITIES = (0.5, 0.1, 0.02, 0.005, 0.001)
SHAPES = ((1_000_000, 1_000), (100_000, 10_000))


def draw_matrix(P, I, density, gen, dev):
    """(right bool [P, I], observed bool [P, I]) on the device, drawn in person slices."""
    right = torch.empty(P, I, dtype=torch.bool, device=dev)
    observed = torch.empty(P, I, dtype=torch.bool, device=dev)
    step = max(1, 200_000_000 // I)
    for s in range(0, P, step):
        n = min(P, s + step) - s
        observed[s:s + n] = torch.rand(n, I, device=dev, generator=gen) < density
        right[s:s + n] = torch.rand(n, I, device=dev, generator=gen) < 0.5
    return right, observed


def problem(P, I, gen, dev):
    D = ops.item_feat_dim(IRT, A)
    return (torch.randn(2, 2 * A, device=dev, generator=gen) * 0.5, torch.randn(I, D, device=dev, generator=gen),
            torch.randn(P, A, device=dev, generator=gen))


def time_blocks(legs, blocks, target_s):
    """legs: {name: callable}.  -> {name: [per-launch ms of each block]}; the legs alternate block by block."""
    iters = {}
    for name, fn in legs.items():          # warm-up, and the launches per block from its time
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        iters[name] = max(2, min(50, int(target_s / max(time.perf_counter() - t0, 1e-5))))
    out = {name: [] for name in legs}
    for _ in range(blocks):
        for name, fn in legs.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters[name]):
                fn()
            stop.record()
            torch.cuda.synchronize()
            out[name].append(start.elapsed_time(stop) / iters[name])
    return out


def worst_disagreement(a, b, item_shape):
    """The legs' outputs against compare_raw's bounds -> (ok, text of the worst ratio error / bound)."""
    worst = []

    def head(name, x, y, tol=2e-5):
        worst.append((abs(float(x) - float(y)) / (tol * max(1.0, abs(float(y)))), name))

    sa, sb = a.scalars.double().cpu(), b.scalars.double().cpu()
    for name, k in (('ll', _lib.S_LL), ('reg', _lib.S_REG), ('kl', _lib.S_KL), ('logq0', _lib.S_LOGQ0), ('logp', _lib.S_LOGP)):
        head(name, sa[k], sb[k])
    head('nobs', sa[_lib.S_NOBS], sb[_lib.S_NOBS], 1e-6)          # (fp32 heads: an exact count rounds once, a summed one a few times)
    for name in ('ability_mu', 'ability_logvar', 'ability'):
        x, y = getattr(a, name), getattr(b, name)
        worst.append((float((x - y).abs().max()) / (2e-5 * max(1.0, float(y.abs().max()))), name))
    for name, x, y in (('g_table[0]', a.grad_table(0), b.grad_table(0)), ('g_table[1]', a.grad_table(1), b.grad_table(1)),
                       ('g_item', a.grad_item(item_shape), b.grad_item(item_shape))):
        worst.append((float((x.double() - y.double()).abs().max()) / (1e-4 * max(float(y.double().abs().max()), 1e-30)), name))
    ratio, name = max(worst)
    return ratio < 1.0, f'{name} at {ratio:.2f} of its bound'


def fmt_ms(ts):
    return f'{statistics.median(ts):9.3f} ({min(ts):.3f} - {max(ts):.3f})'


GATHER_SHAPE = (100_000, 10_000)
GATHER_DENSITIES = (0.02, 0.001)
GATHER_BATCHES = (1_024, 16_384, None)          # None: every person


def gathered_table(args, dev, gen, spec):
    """The --gathered table's lines (see the docstring)."""
    D = spec.item_dim
    P, I = max(64, int(GATHER_SHAPE[0] * args.scale)), GATHER_SHAPE[1]
    table, item, eps = problem(P, I, gen, dev)
    lines = [f'{"shape":>16} {"density":>8} {"cells":>12} {"B":>7} {"batch cells":>12} | {"gather leg ms":>28} {"range leg ms":>28} '
             f'{"codes leg (row_index) ms":>28} | {"column side MB":>14} | gather agrees with codes']
    for density in GATHER_DENSITIES:
        right, observed = draw_matrix(P, I, density, gen, dev)
        codes_t = torch.where(observed, right.to(torch.uint8), torch.full((), 2, dtype=torch.uint8, device=dev))
        padded = torch.full((P, (I + 15) // 16 * 16), 2, dtype=torch.uint8, device=dev)
        padded[:, :I] = codes_t
        codes = ops.CellCodes(padded[:, :I])
        rows = SparseRows._from_observed(observed, right)
        del right, observed, codes_t
        for B in GATHER_BATCHES:
            B = P if B is None else min(B, P)
            idx = torch.randperm(P, device=dev, generator=gen)[:B].contiguous()
            view, start, e = rows.take(idx), (P - B) // 2, eps[:B].contiguous()
            block = rows.rows(range(start, start + B))

            def gather_leg():
                return sparse._hip_sparse_elbo(spec, view, table, item, e, _lib.REG_KL, True)

            def range_leg():
                return sparse._hip_sparse_elbo(spec, block, table, item, e, _lib.REG_KL, True)

            def codes_leg():
                return ops._hip_launch_elbo(spec, codes.codes, codes.codes, _lib.MASK_CODES, idx, table, item, e, None, _lib.REG_KL, True, B)

            ok, why = worst_disagreement(gather_leg(), codes_leg(), (I, D))
            torch.cuda.synchronize()
            t = time_blocks({'gather': gather_leg, 'range': range_leg, 'codes': codes_leg}, args.blocks, args.block_seconds)
            batch_cells = int((rows.row_ptr[idx + 1] - rows.row_ptr[idx]).sum())
            lines.append(f'{f"{P} x {I}":>16} {density:8.3%} {rows.nnz:12d} {B:7d} {batch_cells:12d} | '
                         f'{fmt_ms(t["gather"]) if ok else "outputs differ":>28} {fmt_ms(t["range"]):>28} {fmt_ms(t["codes"]):>28} | '
                         f'{4 * rows.nnz / 1e6:14.1f} | {"yes" if ok else "NO"}: {why}')
            print(lines[-1], flush=True)
        assert rows.bad_index_count == 0 and bool((rows.slot_map() == _lib.SPARSE_NO_SLOT).all())
        del codes, padded, rows
        torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per leg, alternating (at least 5)')
    ap.add_argument('--block-seconds', type=float, default=0.15, help='launches per block are sized to about this long')
    ap.add_argument('--scale', type=float, default=1.0, help='scale every person count (rehearsals; the record is taken at 1.0)')
    ap.add_argument('--skip-wide', action='store_true', help='leave out the 1M x 100k sparse-only row')
    ap.add_argument('--gathered', action='store_true', help='the gathered-minibatch table instead (gather / range / codes legs at 100k x 10k)')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('sparse_crossover: no GPU -- nothing is measured without one')
    if args.blocks < 5:
        raise SystemExit('sparse_crossover: at least 5 blocks')
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    spec = ops.ElboSpec(irt_model=IRT, ability_dim=A)
    D = spec.item_dim
    if args.gathered:
        lines = ['command: python tools/sparse_crossover.py ' + ' '.join(sys.argv[1:] if argv is None else argv),
                 f'device: {torch.cuda.get_device_name(0)}; 2PL, ability_dim {A}, forward + backward, VIBO_SPARSE_CHUNK {_lib.SPARSE_CHUNK}',
                 'ms per launch: median (min - max) over %d alternating blocks' % args.blocks, ''] + gathered_table(args, dev, gen, spec)
        text = '\n'.join(lines) + '\n'
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write(text)
        return
    lines = ['command: python tools/sparse_crossover.py ' + ' '.join(sys.argv[1:] if argv is None else argv),
             f'device: {torch.cuda.get_device_name(0)}; 2PL, ability_dim {A}, forward + backward, VIBO_SPARSE_CHUNK {_lib.SPARSE_CHUNK}',
             'ms per launch: median (min - max) over %d alternating blocks' % args.blocks,
             '',
             f'{"shape":>16} {"density":>8} {"cells":>12} | {"dense leg (codes) ms":>32} {"kernel":>28} {"B/cell":>7} | '
             f'{"sparse leg ms":>32} {"B/cell":>9} {"Gcell/s":>8} {"GB/s streamed":>13} | outputs agree']
    below = {}
    for P0, I in SHAPES:
        P = max(64, int(P0 * args.scale))
        table, item, eps = problem(P, I, gen, dev)
        for density in DENSITIES:
            right, observed = draw_matrix(P, I, density, gen, dev)
            codes_t = torch.where(observed, right.to(torch.uint8), torch.full((), 2, dtype=torch.uint8, device=dev))
            stride = (I + 15) // 16 * 16
            padded = torch.full((P, stride), 2, dtype=torch.uint8, device=dev)
            padded[:, :I] = codes_t
            codes = ops.CellCodes(padded[:, :I])
            rows = SparseRows._from_observed(observed, right)
            del right, observed, codes_t
            kernel = ops.plan_kernel(spec, P, I, _lib.MASK_CODES, True)

            def dense_leg():
                return ops._hip_launch_elbo(spec, codes.codes, codes.codes, _lib.MASK_CODES, None, table, item, eps, None, _lib.REG_KL, True, P)

            def sparse_leg():
                return sparse._hip_sparse_elbo(spec, rows, table, item, eps, _lib.REG_KL, True)

            ok, why = worst_disagreement(sparse_leg(), dense_leg(), (I, D))
            torch.cuda.synchronize()
            t = time_blocks({'dense': dense_leg, 'sparse': sparse_leg}, args.blocks, args.block_seconds)
            med = statistics.median(t['sparse']) * 1e-3
            shape = f'{P} x {I}'
            lines.append(f'{shape:>16} {density:8.3%} {rows.nnz:12d} | {fmt_ms(t["dense"]):>32} {kernel[:28]:>28} {1 / rows.density:7.1f} | '
                         f'{fmt_ms(t["sparse"]) if ok else "outputs differ":>32} {12:3d}+{4 * (D + A):<5d} {rows.nnz / med * 1e-9:8.2f} '
                         f'{12 * rows.nnz / med * 1e-9:13.1f} | {"yes" if ok else "NO"}: {why}')
            if ok and max(t['sparse']) < min(t['dense']):
                below.setdefault(shape, []).append(density)
            print(lines[-1], flush=True)
            del codes, padded, rows
            torch.cuda.empty_cache()
    if not args.skip_wide:
        P, I, per_row = max(64, int(1_000_000 * args.scale)), 100_000, 32
        table, item, eps = problem(P, I, gen, dev)
        key = torch.unique(torch.arange(P, device=dev).repeat_interleave(per_row) * I + torch.randint(0, I, (P * per_row,), device=dev, generator=gen))
        rows = SparseRows.from_coo(key // I, key % I, torch.rand(key.numel(), device=dev, generator=gen) < 0.5, P, I, check=False)
        del key
        t = time_blocks({'sparse': lambda: sparse._hip_sparse_elbo(spec, rows, table, item, eps, _lib.REG_KL, True)}, args.blocks, args.block_seconds)
        med = statistics.median(t['sparse']) * 1e-3
        lines.append(f'{f"{P} x {I}":>16} {rows.density:8.3%} {rows.nnz:12d} | {"no dense leg (above 32767 items)":>32} {"-":>28} {"-":>7} | '
                     f'{fmt_ms(t["sparse"]):>32} {12:3d}+{4 * (D + A):<5d} {rows.nnz / med * 1e-9:8.2f} {12 * rows.nnz / med * 1e-9:13.1f} | '
                     f'no comparator at this size (the suite holds 300 x 40000 to the fp64 oracle)')
        print(lines[-1], flush=True)
    lines.append('')
    for P0, I in SHAPES:
        shape = f'{max(64, int(P0 * args.scale))} x {I}'
        ds = below.get(shape, [])
        # the largest measured density from which every smaller measured one is wholly below as well
        good = None
        for d in sorted(DENSITIES):
            if d in ds:
                good = d
            else:
                break
        lines.append(f'{shape}: ' + (f'the sparse leg\'s range lies wholly under the dense leg\'s at every measured density <= {good:.3%}'
                                     if good is not None else 'no measured density at which the sparse leg\'s range lies wholly under the dense leg\'s'))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
