"""Generate the NLSPN source-model and BatchNorm-adaptation-baseline golden vectors by running the REAL reference on the CPU (where
make_golden_nlspn.py finds it).

The shims, the frames and the call pattern are make_golden_nlspn.py's (imported from it: the reference is imported in place, nothing of it is
copied); the weight helpers are tests/nlspn_meta_cases.py's.  What differs is the driven network: NLSPNModel_Adapt WITHOUT `_prepare_head`, whose
forward with loss_type 'pretrain' (the reference's default) is `_forward` (nlspnmodel_adapt.py:502-509, :792-848) -- conv1_rgb feeds fe1
directly, one pass, no zero-image pass, no heads.
  Source model ("pre-trained" row): the eval forward of the loaded checkpoint; every BatchNorm2d normalises with its loaded running statistics.
  BatchNorm-adaptation baseline: adapt_parameters('meta_bn') on that model finds no 'meta' parameter -- gamma / beta of every BatchNorm2d adapt
    (86 tensors), the running statistics are dropped (src/nlspn_model_adapt.py:322-337).  One step = forward(loss_type 'pretrain_bn') ->
    (depth, None, None), compute_loss(loss_type='adapt') with embedding = reference = None (loss_cos = 0, src/external_model_adapt.py:420-427),
    backward, torch.optim.Adam.step; then the eval forward, which normalises with batch statistics.
Weights: gamma / beta far from (1, 0) (nlspn_meta_cases.meta_state_dict); running statistics = the source model's own activation statistics on
frame 0 at 32x64 (`calibrate`: one train-mode `_forward`, momentum None), moved away per channel by perturb_stats.  Stored once, in
nlspn_source_32x64.npz (`bn/<name>`).
Asserted here, on the CPU:
  * the baseline's adapted names are the 88-entry 'meta_bn' list minus the two meta tensors, in order;
  * loss_cos is 0 in every step;
  * the running-statistics eval differs from a batch-statistics eval of the same weights by more than 1e-2 relative MAE;
  * no BatchNorm2d buffer changes (source: the loaded buffers are what they were; baseline: they stay dropped, no step is counted).
The first-step fixtures also hold the 86 gradients of the same step evaluated by the reference in float64 (`s0/grad64/<name>`, stored as
float32): the deep BatchNorm2d of a 32x64 frame normalise over 8 pixels, and the reference's own float32 gradients sit up to 1e-1 of the
largest entry from them -- the floor any float32 engine's gradient error is read against.
The six-frame fixture also holds the reference against ITSELF with one adapted gamma entry moved one ulp (`alt_rel_mae`).
Holes (exact zeros of the clamped eval output) are left as they are and counted (`n_zero_eval`), as in make_golden_nlspn_meta.py.
Usage:  python tests/golden/make_golden_nlspn_source.py
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tta-depth-completion_amd'))
import make_golden_nlspn as G  # noqa: E402
from proxytta import synth  # noqa: E402
from proxytta.nlspn import nlspn_adapted_names  # noqa: E402
from tests.nlspn_meta_cases import PREPARE, bn2d_prefixes, perturb_stats  # noqa: E402
from tests.nlspn_source_cases import BASELINE_FIRST, BASELINE_SEQ, SOURCE_EVAL, baseline_names, source_state_dict  # noqa: E402

EVAL_TYPE = 'pretrain'              # the reference's default loss_type
TRAIN_TYPE = 'pretrain_bn'          # 'bn' in the string: the training forward returns (depth, None, None)


def rel_mae(a, b):
    return float((a - b).abs().mean() / b.abs().mean())


def source_model(ema, hp, stats, offset=False):
    """ExternalModel_Adapt('nlspn') as constructed, never prepared, with the fixtures' weights."""
    model = ema.ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=hp['max_input_depth'], offset=offset, device=torch.device('cpu'))
    net = model.model.model
    sd = source_state_dict(stats)
    assert list(sd.keys()) == list(net.state_dict().keys()), 'key table drifted from reference'
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model, net, sd


def calibrate(ema, hp):
    model, net, sd = source_model(ema, hp, {})
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = None
            m.reset_running_stats()
    raw, image1, sparse_np = G.nlspn_frame(0, 32, 64, 1)
    model.train()
    with torch.no_grad():
        model.forward(image=torch.from_numpy(image1), sparse_depth=torch.from_numpy(sparse_np), loss_type=TRAIN_TYPE)
    now = net.state_dict()
    stats = {}
    for pre in bn2d_prefixes(sd):
        assert int(now[pre + '.num_batches_tracked']) == 1, pre         # ONE pass: no proxy pass in `_forward`
        stats[pre + '.running_mean'], stats[pre + '.running_var'] = perturb_stats(pre, now[pre + '.running_mean'].numpy(), now[pre + '.running_var'].numpy())
    return stats


def header(h, w, n, steps, hp, offset):
    return {'meta': np.array([h, w, n, steps], dtype=np.int64),
            'hp': np.array([hp['lr'], hp['betas'][0], hp['betas'][1], hp['eps'], hp['weight_decay'], hp['w_sd'], hp['w_sm'],
                            hp['w_cos'], hp['max_input_depth']], dtype=np.float64),
            'legacy': np.array(int(offset))}


def run_source(ema, h, w, n, hp, stats, offset=False):
    model, net, sd = source_model(ema, hp, stats, offset)
    buffers0 = {k: v.clone() for k, v in net.state_dict().items()}
    raw, image1, sparse_np = G.nlspn_frame(0, h, w, n)
    image, sparse = torch.from_numpy(image1), torch.from_numpy(sparse_np)
    model.eval()
    with torch.no_grad():
        depth = model.forward(image=image, sparse_depth=sparse, loss_type=EVAL_TYPE)
    out = header(h, w, n, 0, hp, offset)
    out['depth_eval'] = depth.numpy()
    out['n_zero_eval'] = np.array(int((depth == 0).sum()))
    twin = copy.deepcopy(model)
    for m in twin.model.model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean = None
            m.running_var = None
    twin.eval()
    with torch.no_grad():
        d_batch = twin.forward(image=image, sparse_depth=sparse, loss_type=EVAL_TYPE)
    out['batch_stat_eval_rel_mae'] = np.array(rel_mae(d_batch, depth))
    assert out['batch_stat_eval_rel_mae'] > 1e-2, out['batch_stat_eval_rel_mae']
    now = net.state_dict()
    assert list(now.keys()) == list(buffers0.keys()) and all(torch.equal(v, now[k]) for k, v in buffers0.items()), 'the eval forward wrote a tensor'
    return out


def run_baseline(ema, h, w, n, steps, hp, stats, offset=False, ulp=False):
    model, net, sd = source_model(ema, hp, stats, offset)
    params = model.adapt_parameters(mode='meta_bn')
    pnames = {id(p): k for k, p in net.named_parameters()}
    names = [pnames[id(p)] for p in params]
    full = nlspn_adapted_names([k for k, _ in synth.nlspn_keys(PREPARE)])
    assert len(full) == 88 and names == [k for k in full if not k.startswith('conv1_rgb_meta')] == baseline_names(sd) and len(names) == 86, names[:4]
    if ulp:
        with torch.no_grad():
            params[0].view(-1)[0] = torch.nextafter(params[0].view(-1)[0], torch.tensor(float('inf')))
    opt = torch.optim.Adam(params, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])
    frozen0 = {k: v.detach().clone() for k, v in net.named_parameters() if k not in names}
    nbt0 = {k: v.clone() for k, v in net.state_dict().items() if k.endswith('num_batches_tracked')}
    out = header(h, w, n, steps, hp, offset)
    out['adapted_names'] = np.array(names)
    for s in range(steps):
        raw, image1, sparse_np = G.nlspn_frame(s, h, w, n)
        image, sparse, loss_image = torch.from_numpy(image1), torch.from_numpy(sparse_np), torch.from_numpy(raw)
        validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
        model.train()
        depth, emb, ref = model.forward(image=image, sparse_depth=sparse, loss_type=TRAIN_TYPE)
        assert emb is None and ref is None
        loss, info = model.compute_loss(
            input_rgb=loss_image, output_depth=depth, sparse_depth=sparse.detach(), validity_map=validity.detach(),
            embedding=emb, reference=ref, w_loss_sparse_depth=hp['w_sd'], w_loss_smoothness=hp['w_sm'],
            w_loss_cos=hp['w_cos'], loss_type='adapt')
        assert float(torch.as_tensor(info['loss_cos'])) == 0.0
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        assert all(k in grads for k in names), 'an adapted tensor got no gradient'
        opt.step()
        model.eval()
        with torch.no_grad():
            depth_eval = model.forward(image=image, sparse_depth=sparse, loss_type=EVAL_TYPE)
        p = 's%d/' % s
        out[p + 'depth_eval'] = depth_eval.numpy()
        out[p + 'n_zero_eval'] = np.array(int((depth_eval == 0).sum()))
        named = dict(net.named_parameters())
        for k in names:
            out[p + 'param/' + k] = named[k].detach().numpy().copy()
        if s == 0:
            out[p + 'depth_train'] = depth.detach().numpy()
            out[p + 'loss_info'] = np.array([float(torch.as_tensor(info[k]).detach()) for k in ('loss', 'loss_smooth', 'loss_sparse_depth', 'loss_cos')])
            for k in names:
                out[p + 'grad/' + k] = grads[k].numpy()
                if steps == 1:
                    out[p + 'exp_avg/' + k] = opt.state[named[k]]['exp_avg'].numpy().copy()
                    out[p + 'exp_avg_sq/' + k] = opt.state[named[k]]['exp_avg_sq'].numpy().copy()
            assert int((depth == 0).sum()) == 0
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            assert m.running_mean is None and m.running_var is None, 'a dropped running statistic came back'
    assert all(torch.equal(v, net.state_dict()[k]) for k, v in nbt0.items()), 'a BatchNorm2d counted a batch'
    assert all(torch.equal(v, dict(net.named_parameters())[k]) for k, v in frozen0.items()), 'a frozen parameter changed'
    return out


def grads_fp64(ema, h, w, n, hp, stats, offset=False):
    """The first step's gradients with the whole network and its inputs in float64."""
    model, net, sd = source_model(ema, hp, stats, offset)
    params = model.adapt_parameters(mode='meta_bn')
    pnames = {id(p): k for k, p in net.named_parameters()}
    net.double()
    raw, image1, sparse_np = G.nlspn_frame(0, h, w, n)
    image, sparse, loss_image = [torch.from_numpy(x).double() for x in (image1, sparse_np, raw)]
    validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
    model.train()
    depth, emb, ref = model.forward(image=image, sparse_depth=sparse, loss_type=TRAIN_TYPE)
    loss, info = model.compute_loss(
        input_rgb=loss_image, output_depth=depth, sparse_depth=sparse, validity_map=validity, embedding=emb, reference=ref,
        w_loss_sparse_depth=hp['w_sd'], w_loss_smoothness=hp['w_sm'], w_loss_cos=hp['w_cos'], loss_type='adapt')
    loss.backward()
    return {'s0/grad64/' + pnames[id(p)]: p.grad.detach().numpy().astype(np.float32) for p in params}


def main():
    ema = G.import_reference()
    G.HOLES['allow'] = True
    torch.manual_seed(0)
    torch.set_num_threads(8)
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sd=1.0, w_sm=2.0, w_cos=0.1, max_input_depth=80.0)
    stats = calibrate(ema, hp)
    # source eval: 32x64, and a size that does not divide by 16 (ceil-halving encoder maps, decoder crops) with a batch and the legacy offsets
    src = [run_source(ema, 32, 64, 1, hp, stats), run_source(ema, 40, 56, 2, hp, stats, offset=True)]
    src[0].update({'bn/' + k: v for k, v in stats.items()})
    for name, o in zip(SOURCE_EVAL, src):
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **o)
        print(name, 'batch-statistics eval vs running-statistics eval rel MAE %.3e' % o['batch_stat_eval_rel_mae'], 'holes:', int(o['n_zero_eval']), flush=True)
    # baseline, first step at the same two shapes
    first = [run_baseline(ema, 32, 64, 1, 1, hp, stats), run_baseline(ema, 40, 56, 2, 1, dict(hp, lr=3e-4), stats, offset=True)]
    first[0].update(grads_fp64(ema, 32, 64, 1, hp, stats))
    first[1].update(grads_fp64(ema, 40, 56, 2, dict(hp, lr=3e-4), stats, offset=True))
    for name, o in zip(BASELINE_FIRST, first):
        worst = max((float(np.abs(o['s0/grad/' + k] - o['s0/grad64/' + k]).max() / np.abs(o['s0/grad64/' + k]).max()), k) for k in o['adapted_names'])
        print(name, 'float32 reference vs float64 reference, worst gradient (max error / max entry): %.3e %s' % worst)
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **o)
        print(name, 'loss', o['s0/loss_info'], 'holes:', int(o['s0/n_zero_eval']), flush=True)
    # six frames at the learning rate the NLSPN scripts run (bash/adapt/adapt_nlspn_vkitti.sh: 3e-4)
    seq = run_baseline(ema, 32, 64, 1, 6, dict(hp, lr=3e-4), stats)
    alt = run_baseline(ema, 32, 64, 1, 6, dict(hp, lr=3e-4), stats, ulp=True)
    seq['alt_rel_mae'] = np.array([rel_mae(torch.from_numpy(alt['s%d/depth_eval' % s]), torch.from_numpy(seq['s%d/depth_eval' % s])) for s in range(6)])
    np.savez_compressed(os.path.join(HERE, BASELINE_SEQ + '.npz'), **seq)
    print(BASELINE_SEQ, 'holes per step:', [int(seq['s%d/n_zero_eval' % s]) for s in range(6)])
    print('reference vs itself, one adapted gamma entry one ulp off, scored depth rel MAE per step:', seq['alt_rel_mae'])


if __name__ == '__main__':
    main()
