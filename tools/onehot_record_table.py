"""VIBO_TOL_RECORD file of tests/test_gpu_onehot_contractions.py -> the table kept in profiles/onehot_contraction_record.txt.

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_onehot_contractions.py -q -m gpu
    python tools/onehot_record_table.py record.jsonl > profiles/onehot_contraction_record.txt
"""
import collections
import json
import re
import sys


def main(path):
    recs = [r for r in map(json.loads, open(path)) if r.get('kind') == 'onehot_contraction']
    worst, count, exact = collections.defaultdict(float), collections.Counter(), collections.Counter()
    for r in recs:
        # Part A: one row per class and pattern over all layouts; Part B: one row per form and pattern over all dims and item counts
        form = re.sub(r' I=\d+ stride=\d+', '', r['form'])
        k = (r['part'], form, r['class'] if r['part'] == 'A' else 'A1..8', r['pattern'], r['observable'] + (' ==' if r.get('exact') else ''))
        worst[k] = max(worst[k], r['ratio'])
        count[k] += 1
        exact[k] += 1 if r.get('exact') else 0
    print(f'Worst error / a-priori bound per form, class, pattern and observable ({len(recs)} records of')
    print('tests/test_gpu_onehot_contractions.py on one MI355X; bounds: oracle/onehot_model.py and the test\'s own counted constants).')
    print('"bit for bit": every comparison of the row was a torch.equal that held.  Part A: all row layouts; Part B: ability_dim 1, 2, 4, 5, 8')
    print('and 63 .. 1500 items in one row.')
    print()
    print(f'{"part":4s} {"form":36s} {"class":8s} {"pattern":10s} {"observable":14s} {"records":>7s} {"worst err/bound":>15s}')
    for k in sorted(worst):
        tail = 'bit for bit' if exact[k] == count[k] and worst[k] == 0 else f'{worst[k]:.3f}'
        print(f'{k[0]:4s} {k[1]:36s} {k[2]:8s} {k[3]:10s} {k[4]:14s} {count[k]:7d} {tail:>15s}')


if __name__ == '__main__':
    main(sys.argv[1])
