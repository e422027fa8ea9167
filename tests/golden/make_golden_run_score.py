"""Golden results of the reference's scoring tails: the REAL eval_utils (src/eval_utils.py), imported in place and run on the CPU, on the
frames of tests/score_cases.py.  Nothing of the reference is copied.  The harness below does what the two drivers do around those calls:
  * adaptation loop (src/tta_main.py:755-809): slice output and ground truth to the window, squeeze, a float mask of gt > 0 zeroed where
    gt < min and where gt > max, the masked pixels of the whole batch handed to eval_utils.torch_* as (1000 x, 1000 y) and
    (0.001 x, 0.001 y); the run keeps `metric * batch_size / 1000` sums (fp32 tensors) and ends with `/ n_sample * 1000`;
  * validate() (:975-1030): the same through numpy with gt > 0, gt > min, gt < max and eval_utils' numpy functions; the run keeps
    `metric * batch_size` per batch in a float64 array and ends with np.sum / n_sample.
tests/golden/run_score.npz holds RESULTS only -- per case and rule the four metrics and the masked count, the run's four numbers per rule
and n_sample -- plus the CRC of every input (a drifting generator is caught) and `worst_rel`: the largest relative difference between
these fp32 results and the exact-sum restatement of tests/score_cases.py, i.e. the reference's own fp32 summation error on these frames.
Usage:  PTTA_REFERENCE=<root of the reference tree> python tests/golden/make_golden_run_score.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import score_cases as C  # noqa: E402

RULES = (C.ADAPT, C.VALIDATE)
RUN_N_SAMPLES = (9, 0, 10)           # 0: the default, the frames the run has seen


def import_eval_utils():
    ref = os.environ.get('PTTA_REFERENCE')
    if not ref or not os.path.isfile(os.path.join(ref, 'src', 'eval_utils.py')):
        raise SystemExit('set PTTA_REFERENCE to the root of the reference tree (it holds src/eval_utils.py)')
    sys.path.insert(0, os.path.join(ref, 'src'))
    import eval_utils
    return eval_utils


def score_adapt(E, out, gt, window, lo, hi):
    wy, wx, wh, ww = window
    o = torch.squeeze(torch.from_numpy(out)[..., wy:wy + wh, wx:wx + ww].clone())
    g = torch.squeeze(torch.from_numpy(gt)[..., wy:wy + wh, wx:wx + ww].clone())
    mask = torch.where(g > 0, torch.ones_like(g), torch.zeros_like(g))
    mask[g < lo] = 0.0
    mask[g > hi] = 0.0
    at = mask.nonzero(as_tuple=True)
    o, g = o[at], g[at]
    return [E.torch_mean_abs_err(1000.0 * o, 1000.0 * g), E.torch_root_mean_sq_err(1000.0 * o, 1000.0 * g),
            E.torch_inv_mean_abs_err(0.001 * o, 0.001 * g), E.torch_inv_root_mean_sq_err(0.001 * o, 0.001 * g)], int(o.numel())


def score_validate(E, out, gt, window, lo, hi):
    wy, wx, wh, ww = window
    o = np.squeeze(out[..., wy:wy + wh, wx:wx + ww])
    g = np.squeeze(gt[..., wy:wy + wh, wx:wx + ww])
    at = np.where(np.logical_and(np.where(g > 0, 1, 0), np.logical_and(g > lo, g < hi)) > 0)
    o, g = o[at], g[at]
    with np.errstate(all='ignore'):
        return [E.mean_abs_err(1000.0 * o, 1000.0 * g), E.root_mean_sq_err(1000.0 * o, 1000.0 * g),
                E.inv_mean_abs_err(0.001 * o, 0.001 * g), E.inv_root_mean_sq_err(0.001 * o, 0.001 * g)], int(o.size)


def run_adapt(E, batches, window, lo, hi, n_sample):
    total = [0.0] * 4
    for out, gt in batches:
        m, _ = score_adapt(E, out, gt, window, lo, hi)
        total = [t + v * out.shape[0] / 1000 for t, v in zip(total, m)]
    return [float(t / n_sample * 1000) for t in total]


def run_validate(E, batches, window, lo, hi, n_sample):
    total = np.zeros((4, len(batches)))
    for k, (out, gt) in enumerate(batches):
        m, _ = score_validate(E, out, gt, window, lo, hi)
        for j in range(4):
            total[j, k] = m[j] * out.shape[0]
    return [float(np.sum(total[j]) / n_sample) for j in range(4)]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(b)
    assert np.array_equal(ok, np.isfinite(a))
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def main():
    E = import_eval_utils()
    score = {C.ADAPT: score_adapt, C.VALIDATE: score_validate}
    run = {C.ADAPT: run_adapt, C.VALIDATE: run_validate}
    metrics = np.zeros((len(C.CASES), 2, 4))
    counts = np.zeros((len(C.CASES), 2), np.int64)
    crcs = np.zeros(len(C.CASES), np.int64)
    worst = 0.0
    for i, c in enumerate(C.CASES):
        out, gt = C.case_frames(c)
        crcs[i] = C.crc(out, gt)
        for j, rule in enumerate(RULES):
            m, counts[i, j] = score[rule](E, out, gt, C.window_of(c), C.LO, C.HI)
            metrics[i, j] = [float(v) for v in m]
            r = C.restate_batch(out, gt, c['window'], rule=rule)
            assert r['count'] == counts[i, j], (c['name'], rule)
            worst = max(worst, rel(r['metrics'], metrics[i, j]))
            print('%-26s %-8s count %6d  %s  rel %.2e' % (c['name'], rule, counts[i, j], metrics[i, j], rel(r['metrics'], metrics[i, j])))
    batches = C.run_frames()
    frames_seen = sum(o.shape[0] for o, _ in batches)
    h, w = C.RUN['size']
    run_metrics = np.zeros((2, len(RUN_N_SAMPLES), 4))
    for j, rule in enumerate(RULES):
        for k, ns in enumerate(RUN_N_SAMPLES):
            run_metrics[j, k] = run[rule](E, batches, (0, 0, h, w), C.LO, C.HI, ns if ns else frames_seen)
            r = C.restate_run(batches, rule=rule, n_sample=ns)
            e = rel([r[m] for m in ('mae', 'rmse', 'imae', 'irmse')], run_metrics[j, k])
            worst = max(worst, e)
            print('%-26s %-8s n_sample %2d  %s  rel %.2e' % (C.RUN['name'], rule, ns, run_metrics[j, k], e))
    print('worst relative difference between the reference\'s fp32 results and the exact-sum restatement: %.3e' % worst)
    np.savez(os.path.join(HERE, 'run_score.npz'), names=np.array([c['name'] for c in C.CASES]), rules=np.array(RULES), metrics=metrics,
             counts=counts, crcs=crcs, run_n_samples=np.array(RUN_N_SAMPLES, np.int64), run_metrics=run_metrics,
             run_crcs=np.array([C.crc(o, g) for o, g in batches], np.int64), worst_rel=np.float64(worst))


if __name__ == '__main__':
    main()
