"""VIBO_TOL_RECORD file of tests/test_gpu_split_worst_case.py -> the table kept in profiles/split_worst_case_record.txt.

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_split_worst_case.py -q -m gpu
    python tools/split_record_table.py record.jsonl > profiles/split_worst_case_record.txt
"""
import collections
import json
import re
import sys


def main(path):
    recs = [r for r in map(json.loads, open(path)) if r.get('kind') == 'split_worst_case']
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


if __name__ == '__main__':
    main(sys.argv[1])
