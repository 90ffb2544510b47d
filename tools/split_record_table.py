"""VIBO_TOL_RECORD file of a cell-by-cell GPU test -> the table kept under profiles/.  The record kind is the second argument:

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_split_worst_case.py -q -m gpu
    python tools/split_record_table.py record.jsonl split_worst_case > profiles/split_worst_case_record.txt

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_narrow_cells.py -q -m gpu
    python tools/split_record_table.py record.jsonl narrow_cells > profiles/narrow_cells_record.txt

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_fallback_cells.py -q -m gpu
    python tools/split_record_table.py record.jsonl fallback_cells > profiles/fallback_cells_record.txt

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_flow_batches.py -q -m gpu
    python tools/split_record_table.py record.jsonl flow_batches >> profiles/flow_batches_record.txt
"""
import collections
import json
import re
import sys


def split_worst_case(recs):
    worst, model = collections.defaultdict(float), collections.defaultdict(float)
    for r in recs:
        k = (r['class'], r['kernel'], r['observable'])
        worst[k] = max(worst[k], r['ratio'])
        if 'model_ratio' in r:
            model[k] = max(model[k], r['model_ratio'])
    print(f'Worst error / a-priori bound per input class, kernel and observable ({len(recs)} records of tests/test_gpu_split_worst_case.py on one')
    print('MI355X; bound: oracle/split_model.py; matrix = split-f16 bound, valu = plain fp32 bound).  "logit": the one observed cell of each')
    print('item, recovered from dLL/db where |l| <= 3.  cpu model: the fp64 model of the documented scheme on the same cells.')
    print()
    print(f'{"class":16s} {"kernel":7s} {"observable":10s} {"worst err/bound":>15s} {"cpu model":>10s}')
    for k in sorted(worst):
        print(f'{k[0]:16s} {k[1]:7s} {k[2]:10s} {worst[k]:15.3f} {model[k]:10.3f}' if k in model else f'{k[0]:16s} {k[1]:7s} {k[2]:10s} {worst[k]:15.3f}')
    print()
    print('Mixed magnitudes in one panel (matrix kernel, observed cells with |l| <= 3): the bound against the plain fp32 bound')
    print('(A + 5) 2^-24 (sum|a theta| + |b|) of the same cell -- what one outlier item costs every ordinary item -- and the kernel on it.')
    print(f'{"case":60s} {"bound/fp32 median":>17s} {"max":>9s} {"kernel err/bound":>17s} {"kernel worst err":>17s}')
    for r in recs:
        if r['class'].startswith('mixed') and 'bound_over_fp32_median' in r:
            cid = re.search(r'\[(.*)-matrix\]', r['test']).group(1)
            print(f'{cid:60s} {r["bound_over_fp32_median"]:17.1f} {r["bound_over_fp32_max"]:9.1f} {r["ratio"]:17.3f} {r["err"]:17.2e}')


def narrow_cells(recs):
    parts = ('sweep', 'sweep-forward', 'units', 'dense')
    worst = collections.defaultdict(float)
    for r in recs:
        worst[(r['part'], r['class'], r['observable'])] = max(worst[(r['part'], r['class'], r['observable'])], r['ratio'])
    obs = sorted({k[2] for k in worst})
    print(f'Worst error / a-priori bound per part, input class and observable ({len(recs)} records of tests/test_gpu_narrow_cells.py on one MI355X;')
    print('bounds: oracle/narrow_model.py).  sweep: all item counts 4..128, ability_dim 1..4, three row modes (/drop: --drop-missing at')
    print('ability_dim 3); sweep-forward: the forward-only launches of the same cases; units: 32 645 persons, one observer per item, at the')
    print('first unit, a later unit and the ragged end; dense: 32 645 persons, 30 % missing, summed bounds with the counted chain.')
    print('S_NOBS is exact or the ratio is infinite.')
    print()
    for part in parts:
        classes = sorted({k[1] for k in worst if k[0] == part})
        if not classes:
            continue
        print(f'{part:14s} ' + ' '.join(f'{c:>13s}' for c in classes))
        for o in obs:
            if any((part, c, o) in worst for c in classes):
                print(f'  {o:12s} ' + ' '.join(f'{worst[(part, c, o)]:13.3f}' if (part, c, o) in worst else f'{"-":>13s}' for c in classes))
        print()


def fallback_cells(recs):
    parts = ('edges', 'encode', 'trips', 'dense')
    worst, trips = collections.defaultdict(float), {}
    for r in recs:
        worst[(r['part'], r['kernel'], r['observable'])] = max(worst[(r['part'], r['kernel'], r['observable'])], r['ratio'])
        if r['part'] not in ('edges', 'encode'):
            trips[r['case']] = r['trips']
    kernels = ('tiled', 'wave-per-row', 'wave-per-person')
    obs = sorted({k[2] for k in worst})
    print(f'Worst error / a-priori bound per part, kernel and observable ({len(recs)} records of tests/test_gpu_fallback_cells.py on one MI355X;')
    print('bounds: oracle/fallback_model.py).  edges: one trip, every waves / chunk / LDS boundary; trips: every workgroup or wave takes')
    print('two trips or more through its persistent loop, one observer per item, at the first trip, a later one and the ragged end;')
    print('dense: 30 % missing, summed bounds with the counted chain; encode: encode_kernel through ops.encode_posterior on the edge rows,')
    print('against its own bound and against the ELBO launch within the summed bounds.  S_NOBS is exact or the ratio is infinite.')
    print()
    for part in parts:
        print(f'{part:22s} ' + ' '.join(f'{k:>16s}' for k in kernels))
        for o in obs:
            if any((part, k, o) in worst for k in kernels):
                print(f'  {o:22s} ' + ' '.join(f'{worst[(part, k, o)]:16.3f}' if (part, k, o) in worst else f'{"-":>16s}' for k in kernels))
        print()
    print('Trips per workgroup (tiled) or wave of the multi-trip launches, (fewest, most), from the geometry functions:')
    for cid in sorted(trips):
        print(f'  {cid:70s} {tuple(trips[cid])}')


def flow_batches(recs):
    fam = lambda r: ('matrix' if r['kernel'] == 'matrix' else 'valu') + (' forward-only' if 'forward-only' in r['case'] else '')
    worst, where = collections.defaultdict(float), {}
    for r in recs:
        k = (fam(r), r['observable'])
        if r['ratio'] >= worst[k]:
            worst[k], where[k] = r['ratio'], (r['err'], r['tol'], r['case'])
    fams = sorted({k[0] for k in worst})
    print(f'Worst observed error per case family and observable ({len(recs)} records of tests/test_gpu_flow_batches.py on one MI355X):')
    print('the error in the units of its bound, the bound, the share of the bound, the case.  Scalars: relative (of max(1, |ref|) but for')
    print('S_LL); ability_mu / logvar / ability: of max(1, max|ref|); ability_k / ability_ladj: absolute; g_flow block: of the block\'s')
    print('max_e sum_batches |batch contribution| (oracle/vibo_table_ref.py fused_elbo_ref_sliced).')
    print()
    for f in fams:
        print(f)
        for o in sorted({k[1] for k in worst if k[0] == f}):
            e, t, cid = where[(f, o)]
            print(f'  {o:18s} {e:10.2e} {t:8.0e} {worst[(f, o)]:7.3f}  {cid}')
        print()


KINDS = {'flow_batches': flow_batches, 'split_worst_case': split_worst_case, 'narrow_cells': narrow_cells, 'fallback_cells': fallback_cells}


def main(path, kind='split_worst_case'):
    KINDS[kind]([r for r in map(json.loads, open(path)) if r.get('kind') == kind])


if __name__ == '__main__':
    main(*sys.argv[1:3])
