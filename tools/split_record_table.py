"""VIBO_TOL_RECORD file of a cell-by-cell GPU test -> the table kept under profiles/.  The record kind is the second argument:

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_split_worst_case.py -q -m gpu
    python tools/split_record_table.py record.jsonl split_worst_case > profiles/split_worst_case_record.txt

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_narrow_cells.py -q -m gpu
    python tools/split_record_table.py record.jsonl narrow_cells > profiles/narrow_cells_record.txt

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_fallback_cells.py -q -m gpu
    python tools/split_record_table.py record.jsonl fallback_cells > profiles/fallback_cells_record.txt

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_flow_batches.py -q -m gpu
    python tools/split_record_table.py record.jsonl flow_batches >> profiles/flow_batches_record.txt

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_decoder_cells.py -q -m gpu
    python tools/split_record_table.py record.jsonl decoder_cells > profiles/decoder_cells_record.txt
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


def decoder_cells(recs):
    order = ('unit', 'hostile', 'cancel', 'small_w', 'small_g', 'large', 'elu0', 'zero', 'guess3')      # oracle/decoder_model.py CLASSES
    parts = ('term', 'single', 'dense')
    worst, grade = collections.defaultdict(float), {}
    probes, seconds, other = [], None, collections.defaultdict(float)
    for r in recs:
        if r['part'] == 'time':
            seconds = r['err']
        elif r['part'] == 'split8-probe':
            probes.append(r)
        elif r['observable'].startswith('bound/fp32 '):
            k = (r['class'], r['observable'][11:])
            g = grade.get(k, (0.0, 0.0))
            grade[k] = (max(g[0], r['median']), max(g[1], r['p95']))
        elif r['part'] in parts:
            worst[(r['part'], r['class'], r['observable'])] = max(worst[(r['part'], r['class'], r['observable'])], r['ratio'])
        else:
            other[(r['part'], r['observable'])] = max(other[(r['part'], r['observable'])], r['ratio'])
    classes = [c for c in order if any(k[1] == c for k in worst)]
    print(f'Worst error / a-priori bound per mask layout, input class and observable ({len(recs)} records of tests/test_gpu_decoder_cells.py on one')
    print('MI355X; bounds: oracle/decoder_model.py).  term: one observed item per (person, 16-item wave group); single: one observed term per')
    print('(person chunk, wave), "x|dz2": the backward half on the kernel\'s own dz2 (dvec_part row 0), split residual evaluated; dense: 30 %')
    print('missing, summed bounds with the counted chains.  Shapes I in {1, 15, 16, 17, 63, 64, 65, 130}, B in {1, 2, 3, 7, 8, 9, 10}, person')
    print('chunks 1, 2, ceil(B / 2), 4.  0 = bit for bit / exactly zero where the line says so; inf would be an entry outside a zero bound.')
    print()
    for part in parts:
        print(f'{part:34s} ' + ' '.join(f'{c:>9s}' for c in classes))
        for o in sorted({k[2] for k in worst if k[0] == part}):
            print(f'  {o:32s} ' + ' '.join(f'{worst[(part, c, o)]:9.3f}' if (part, c, o) in worst else f'{"-":>9s}' for c in classes))
        print()
    print('Other parts (class unit): worst error / bound per observable')
    for p in sorted({k[0] for k in other}):
        print(f'  {p:14s} ' + '  '.join(f'{o} {other[(p, o)]:.3f}' for (q, o) in sorted(other) if q == p))
    print()
    print('The three contractions\' own bounds (representation of the pieces, the dropped lo x lo, accumulation; nothing propagated) over the')
    print('bound of a plain fp32 evaluation of the same sum (decoder_model.fp32_grade), on observed terms with a live gradient: median and')
    print('95th percentile over the entries, the largest over the cases.  About 1: "fp32-grade".  z2 = W2 . h1 (64 products), dH1 = W2^T . dz2')
    print('(64 products), dW2: ONE outer product dz2[n] h1[k] against one fp32 multiplication.')
    print(f'{"class":10s} ' + ' '.join(f'{n + " median":>14s} {n + " p95":>12s}' for n in ('z2', 'dH1', 'dW2')))
    for c in classes:
        print(f'{c:10s} ' + ' '.join((f'{grade[(c, n)][0]:14.3g} {grade[(c, n)][1]:12.3g}' if (c, n) in grade else f'{"-":>14s} {"-":>12s}') for n in ('z2', 'dH1', 'dW2')))
    print()
    print('split8 on the device (h1 = (1, 0) | (1, 2^-11) in pieces exactly: dW2_part[n][even k] = hi + lo and dW2_part[n][odd k] - dW2_part[n][even k] =')
    print('2^-11 hi of dz2[n] = dvec_part[0][n]): dz2 values whose two pieces both equal the model that keeps f16 subnormals / one whose conversion')
    print('flushes a subnormal hi, the largest residual |hi + lo - dz2|, pieces on the subnormal grid.')
    print(f'{"scale":30s} {"entries":>8s} {"= model":>8s} {"= flushing":>10s} {"device residual":>16s} {"model residual":>15s} {"subnormal lo":>13s} {"subnormal hi":>13s}')
    for r in probes:
        print(f'{r["class"]:30s} {r["entries"]:8d} {r["equal_to_model"]:8d} {r["equal_to_flushing_model"]:10d} {r["err"]:16.3e} {r["model_residual"]:15.3e} '
              f'{r["subnormal_lo"]:13d} {r["subnormal_hi"]:13d}')
    if seconds is not None:
        print()
        print(f'The whole file: {seconds:.0f} s.')


KINDS = {'flow_batches': flow_batches, 'split_worst_case': split_worst_case, 'narrow_cells': narrow_cells, 'fallback_cells': fallback_cells,
         'decoder_cells': decoder_cells}


def main(path, kind='split_worst_case'):
    KINDS[kind]([r for r in map(json.loads, open(path)) if r.get('kind') == kind])


if __name__ == '__main__':
    main(*sys.argv[1:3])
