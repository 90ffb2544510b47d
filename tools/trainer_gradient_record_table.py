"""VIBO_TOL_RECORD file of tests/test_gpu_trainer_gradients.py -> the table kept in profiles/r07_trainer_gradient_record.txt.

    VIBO_TOL_RECORD=record.jsonl python -m pytest tests/test_gpu_trainer_gradients.py -q -m gpu
    python tools/trainer_gradient_record_table.py record.jsonl > profiles/r07_trainer_gradient_record.txt
"""
import collections
import json
import sys


def trainer_of(what):
    for word, name in (('decoder', 'FusedDecoderTrainer'), ('cond/flow', 'FusedCondFlowTrainer'), ('mean', 'FusedMeanTrainer')):
        if what.startswith(word) or word in what.lower():
            return name
    return {'FusedCondFlowTrainer': 'FusedCondFlowTrainer', 'FusedMeanTrainer': 'FusedMeanTrainer',
            'FusedDecoderTrainer': 'FusedDecoderTrainer'}.get(what, 'FusedTrainer')


def main(path):
    recs = list(map(json.loads, open(path)))
    grads = [r for r in recs if r.get('kind') == 'trainer_grad']
    worst, count = collections.defaultdict(float), collections.Counter()
    for r in grads:
        k = (trainer_of(r['what']), r['family'], r['tol'])
        worst[k] = max(worst[k], r['err'])
        count[k] += 1
    print(f'Worst gradient error per trainer and tensor family ({len(grads)} tensors x steps of tests/test_gpu_trainer_gradients.py on one MI355X):')
    print('max|g - g64| / max|g64|, g read back from Adam\'s first moment, g64 the fp64 oracle at the parameters the step started from.')
    print()
    print(f'{"trainer":22s} {"tensor family":15s} {"tensors":>8s} {"worst error":>12s} {"bound":>8s} {"error / bound":>14s}')
    for k in sorted(worst):
        print(f'{k[0]:22s} {k[1]:15s} {count[k]:8d} {worst[k]:12.2e} {k[2]:8.0e} {worst[k] / k[2]:14.3f}')
    gold = [r for r in recs if r.get('kind') == 'trainer_grad_golden']
    if gold:
        print()
        print(f'The reference\'s recorded gradients (tests/golden/case_*.npz, {len(gold)} tensors): the smaller of the distances to fp64 and to the reference.')
        worst = collections.defaultdict(float)
        for r in gold:
            worst[(r['what'], r['family'])] = max(worst[(r['what'], r['family'])], r['err'] / r['tol'])
        for k in sorted(worst):
            print(f'{k[0]:22s} {k[1]:15s} worst error / bound {worst[k]:8.3f}')
    adam = [r for r in recs if r.get('kind') == 'trainer_adam']
    if adam:
        print()
        print(f'Adam\'s update from the kernel\'s own moments ({len(adam)} buffers x steps): worst |p_t - formula| / (1e-4 lr + 2^-23 |p|) = '
              f'{max(r["ratio"] for r in adam):.3f}, largest absolute error {max(r["err"] for r in adam):.2e}')


if __name__ == '__main__':
    main(sys.argv[1])
