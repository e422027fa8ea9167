"""Generate the NLSPN adapt_mode 'meta' golden vectors by running the REAL reference on the CPU (where make_golden_nlspn.py finds it).

The shims, the frames and the call sequence are make_golden_nlspn.py's (imported from it: the reference is
imported in place, nothing of it is copied); what differs is the driven mode and the weights:
  adapt_parameters('meta') (src/nlspn_model_adapt.py:302-311): conv1_rgb_meta's weight and bias alone adapt; every BatchNorm2d is frozen and
  keeps its loaded buffers with track_running_stats = False -- train-mode passes use batch statistics and write no buffer, the scored eval
  forward (src/tta_main.py:729-736) normalises with the LOADED running statistics and gamma / beta.
  Weights: tests/nlspn_meta_cases.py meta_state_dict() -- gamma / beta far from (1, 0); running statistics = the network's own activation
  statistics on frame 0 (measured here by `calibrate`, on the reference, as a trained checkpoint would hold them) moved away per channel, so
  that they are neither (0, 1) nor any frame's batch statistics.  Stored once, in nlspn_meta_32x64.npz (`bn/<name>`).
Asserted here, on the CPU:
  * the reference's eval depth differs from a batch-statistics eval of the same weights by far more than the tests' bound (> 1e-2 rel MAE);
  * no BatchNorm2d running buffer changes over the six-frame sequence (the heads' BatchNorm1d are not BatchNorm2d: 'meta' leaves them
    tracking, as 'meta_bn' does, and their buffers do move);
  * adapt_parameters('meta_fix') (:313-320) gives bit-identical vectors (asserted once, nothing stored for it).
The six-frame fixture also holds the reference against ITSELF with one adapted weight moved one ulp (`alt_rel_mae`): the sensitivity floor of
its own trajectory, which the scored depth's 1e-3 bound is judged against (DESIGN.md section 10 did the same for the 2layers block).
Holes: with running statistics the eval output of these synthetic frames has a few exact zeros (about a dozen pixels per frame, where the
final clamp cut a negative prediction).  scikit-image is absent here, so -- as for the full-size fixtures of make_golden_nlspn.py -- the holes
are left as they are and counted (`n_zero_eval`): the fixtures pin the eval output BEFORE hole filling, which is what ptta_forward_eval returns.
Usage:  python tests/golden/make_golden_nlspn_meta.py
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
from tests.nlspn_meta_cases import META_NAMES, PREPARE, bn2d_prefixes, is_bn2d, meta_state_dict, perturb_stats  # noqa: E402


def rel_mae(a, b):
    return float((a - b).abs().mean() / b.abs().mean())


def calibrate(ema, hp):
    """Activation statistics of every BatchNorm2d on frame 0 at 32x64 (cumulative average over the grad pass and the proxy pass of one
    train-mode forward, momentum None), then perturb_stats."""
    model = ema.ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=hp['max_input_depth'], offset=False, device=torch.device('cpu'))
    model._prepare_head(PREPARE)
    net = model.model.model
    sd = meta_state_dict(stats={})
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = None
            m.reset_running_stats()
    raw, image1, sparse_np = G.nlspn_frame(0, 32, 64, 1)
    model.train()
    with torch.no_grad():
        model.forward(image=torch.from_numpy(image1), sparse_depth=torch.from_numpy(sparse_np), loss_type=G.LOSS_TYPE)
    now = net.state_dict()
    stats = {}
    for pre in bn2d_prefixes(sd):
        assert int(now[pre + '.num_batches_tracked']) >= 1, pre
        stats[pre + '.running_mean'], stats[pre + '.running_var'] = perturb_stats(pre, now[pre + '.running_mean'].numpy(), now[pre + '.running_var'].numpy())
    return stats


def run_case(ema, h, w, n, steps, hp, stats, offset=False, mode='meta', ulp=False):
    model = ema.ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=hp['max_input_depth'], offset=offset, device=torch.device('cpu'))
    model._prepare_head(PREPARE)
    net = model.model.model
    sd = meta_state_dict(stats)
    assert list(sd.keys()) == list(net.state_dict().keys()), 'key table drifted from reference'
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    params = model.adapt_parameters(mode=mode)
    pnames = {id(p): k for k, p in net.named_parameters()}
    names = [pnames[id(p)] for p in params]
    assert names == META_NAMES, names
    if ulp:
        with torch.no_grad():
            params[0].view(-1)[0] = torch.nextafter(params[0].view(-1)[0], torch.tensor(float('inf')))
    opt = torch.optim.Adam(params, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])
    buffers0 = {k: v.clone() for k, v in net.state_dict().items() if k.endswith(('running_mean', 'running_var'))}
    frozen0 = {k: v.detach().clone() for k, v in net.named_parameters() if k not in names}
    out = {'meta': np.array([h, w, n, steps], dtype=np.int64),
           'hp': np.array([hp['lr'], hp['betas'][0], hp['betas'][1], hp['eps'], hp['weight_decay'], hp['w_sd'], hp['w_sm'],
                           hp['w_cos'], hp['max_input_depth']], dtype=np.float64),
           'adapted_names': np.array(names), 'legacy': np.array(int(offset))}
    for s in range(steps):
        raw, image1, sparse_np = G.nlspn_frame(s, h, w, n)
        image, sparse, loss_image = torch.from_numpy(image1), torch.from_numpy(sparse_np), torch.from_numpy(raw)
        validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
        model.train()
        depth, emb, ref = model.forward(image=image, sparse_depth=sparse, loss_type=G.LOSS_TYPE)
        loss, info = model.compute_loss(
            input_rgb=loss_image, output_depth=depth, sparse_depth=sparse.detach(), validity_map=validity.detach(),
            embedding=emb, reference=ref, w_loss_sparse_depth=hp['w_sd'], w_loss_smoothness=hp['w_sm'],
            w_loss_cos=hp['w_cos'], loss_type='adapt')
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        opt.step()
        model.eval()
        with torch.no_grad():
            depth_eval = model.forward(image=image, sparse_depth=sparse, loss_type=G.LOSS_TYPE)
        p = 's%d/' % s
        out[p + 'depth_eval'] = depth_eval.numpy()
        out[p + 'n_zero_eval'] = np.array(int((depth_eval == 0).sum()))
        named = dict(net.named_parameters())
        for k in names:
            out[p + 'param/' + k] = named[k].detach().numpy().copy()
        if steps == 1 or s == 0:
            out[p + 'depth_train'] = depth.detach().numpy()
            out[p + 'loss_info'] = np.array([float(torch.as_tensor(info[k]).detach()) for k in ('loss', 'loss_smooth', 'loss_sparse_depth', 'loss_cos')])
            for k in names:
                out[p + 'grad/' + k] = grads[k].numpy()
            assert int((depth == 0).sum()) == 0
        if s == 0 and not ulp and mode == 'meta':
            # the same weights evaluated with BATCH statistics (what 'meta_bn' does): must be far from the running-statistics eval
            twin = copy.deepcopy(model)
            for m in twin.model.model.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean = None
                    m.running_var = None
            twin.eval()
            with torch.no_grad():
                d_batch = twin.forward(image=image, sparse_depth=sparse, loss_type=G.LOSS_TYPE)
            out['batch_stat_eval_rel_mae'] = np.array(rel_mae(d_batch, depth_eval))
            assert out['batch_stat_eval_rel_mae'] > 1e-2, out['batch_stat_eval_rel_mae']
    now = net.state_dict()
    moved = [k for k, v in buffers0.items() if not torch.equal(v, now[k])]
    assert not [k for k in moved if is_bn2d(k)], 'a BatchNorm2d running buffer changed: %s' % moved[:4]
    assert all(torch.equal(v, dict(net.named_parameters())[k]) for k, v in frozen0.items()), 'a frozen parameter changed'
    out['moved_head_buffers'] = np.array(sorted(moved))
    return out


def same(a, b):
    """every vector of run b bit for bit in run a (a, the 'meta' run, holds the batch-statistics comparison besides)"""
    return set(a) - set(b) == {'batch_stat_eval_rel_mae'} and all(np.array_equal(a[k], b[k]) for k in b)


def main():
    ema = G.import_reference()
    G.HOLES['allow'] = True
    torch.manual_seed(0)
    torch.set_num_threads(8)
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sd=1.0, w_sm=2.0, w_cos=0.1, max_input_depth=80.0)
    stats = calibrate(ema, hp)
    one = run_case(ema, 32, 64, 1, 1, hp, stats)
    assert same(one, run_case(ema, 32, 64, 1, 1, hp, stats, mode='meta_fix')), "'meta_fix' differs from 'meta'"
    one.update({'bn/' + k: v for k, v in stats.items()})
    np.savez_compressed(os.path.join(HERE, 'nlspn_meta_32x64.npz'), **one)
    # a size that does not divide by 16 (decoder crops, nlspnmodel_adapt.py:474-490), batch 2, the legacy offsets src/tta_main.py:309-317 constructs
    two = run_case(ema, 40, 56, 2, 1, dict(hp, lr=3e-4), stats, offset=True)
    np.savez_compressed(os.path.join(HERE, 'nlspn_meta_40x56_n2.npz'), **two)
    # the sequence at the learning rate the NLSPN scripts run (bash/adapt/adapt_nlspn_vkitti.sh: 3e-4).  Adam's first steps move every weight
    # by ~lr whatever the gradient's size, so the reference's own one-ulp sensitivity (`alt`) grows with lr x steps: at 1e-3 it passed 1e-3 in
    # the fifth step (9.3e-5, 3.5e-4, 6.5e-4, 9.1e-4, 1.0e-3, 1.4e-3) and no engine could be held to the north-star bound there
    seq = run_case(ema, 32, 64, 1, 6, dict(hp, lr=3e-4), stats)
    alt = run_case(ema, 32, 64, 1, 6, dict(hp, lr=3e-4), stats, ulp=True)
    seq['alt_rel_mae'] = np.array([rel_mae(torch.from_numpy(alt['s%d/depth_eval' % s]), torch.from_numpy(seq['s%d/depth_eval' % s])) for s in range(6)])
    np.savez_compressed(os.path.join(HERE, 'nlspn_meta_32x64_seq6.npz'), **seq)
    for name, o in (('32x64', one), ('40x56_n2', two), ('32x64_seq6', seq)):
        print('nlspn_meta_' + name, 'loss', o['s0/loss_info'], 'batch-statistics eval vs running-statistics eval rel MAE %.3e' % o['batch_stat_eval_rel_mae'],
              'BatchNorm1d buffers that moved:', len(o['moved_head_buffers']), 'holes per step:', [int(o['s%d/n_zero_eval' % s]) for s in range(int(o['meta'][3]))], flush=True)
    print('reference vs itself, one adapted weight one ulp off, scored depth rel MAE per step:', seq['alt_rel_mae'])


if __name__ == '__main__':
    main()
