"""Golden vectors of the reference's stage-2 head trainer in the form its stage 2 always runs: SyncBatchNorm + DDP.

src/head_main.py:278 calls `model.convert_syncbn()` (and :279 `distributed_data_parallel(rank)`) after the head Adam is built and before
`train(prepare=True)` (:407, :417).  After the conversion train_prepare's isinstance test (BatchNorm2d / SyncBatchNorm) matches every
BatchNorm of the model:
  NLSPN      (src/nlspn_model_adapt.py:360-368)     proj_t.1 goes to eval mode (running statistics, untouched)
  CostDCNet  (src/costdcnet_model_adapt.py:418-430) proj_t.1, UNet3D's BatchNorm3d and the sparse encoder's BatchNorm1d go to eval mode
  MSG_CHN    (src/msg_chn_model_adapt.py:435-440)   train_prepare is train(): one rank computes what the plain form computes
One process, no process group: SyncBatchNorm never synchronises, so the CPU stand-in of make_golden_costdcnet.install_cpu_syncbn is exact.
The batch-2 cases are what two ranks of one frame each must reproduce together (global-batch statistics, mean gradient).
Backbone set-up, frames, target perturbation and sampling are imported from make_golden_head_generic.py / make_golden_head.py.
Usage:  python tests/golden/make_golden_head_syncbn.py [nlspn|costdcnet|msg_chn]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_head_generic as HG  # noqa: E402

CASES = {
    'nlspn': [('head_syncbn_nlspn_forward_48x80', 'head_selfsup_seq_ema', 48, 80, 1, 2),
              ('head_syncbn_nlspn_reverse_48x80', 'head_selfsup_seq_ema_reverse', 48, 80, 1, 2),
              ('head_syncbn_nlspn_reverse_48x80_n2', 'head_selfsup_seq_ema_reverse', 48, 80, 2, 2)],
    'costdcnet': [('head_syncbn_costdcnet_forward_64x96', 'head_selfsup_seq_ema', 64, 96, 1, 2),
                  ('head_syncbn_costdcnet_reverse_64x96', 'head_selfsup_seq_ema_reverse', 64, 96, 1, 2),
                  ('head_syncbn_costdcnet_reverse_64x96_n2', 'head_selfsup_seq_ema_reverse', 64, 96, 2, 2)],
    'msg_chn': [('head_syncbn_msg_chn_forward_32x48', 'head_selfsup_seq_ema', 32, 48, 1, 2),
                ('head_syncbn_msg_chn_reverse_32x48', 'head_selfsup_seq_ema_reverse', 32, 48, 1, 2),
                ('head_syncbn_msg_chn_reverse_32x48_n2', 'head_selfsup_seq_ema_reverse', 32, 48, 2, 2)],
}


def run_case(model, net, sd, frames, name, loss_type, steps, meta, put):
    head_params = model.prepare_parameters('head_selfsup_ema')        # head_main.py:268 (re-creates the heads)
    sd = dict(sd)
    sd.update(HG.perturbed_target(sd))
    assert list(sd.keys()) == list(net.state_dict().keys()), 'key table drifted from reference'
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    names = [k for k, p in net.named_parameters() if any(p is q for q in head_params)]
    assert len(names) == 12, names
    opt = torch.optim.Adam(head_params, **HG.HEAD_HP)                 # head_main.py:270
    import make_golden_costdcnet as MC
    MC.install_cpu_syncbn()
    model.convert_syncbn()                                            # head_main.py:278, where the reference calls it
    # (:279 distributed_data_parallel: with one rank DDP's gradient mean is the identity, and it cannot wrap a CPU model without a group)
    n_sync = sum(isinstance(m, torch.nn.SyncBatchNorm) for m in net.modules())
    assert n_sync > 0, 'convert_syncbn converted nothing'
    out = {'meta': np.array(meta, dtype=np.int64), 'loss_type': np.array(loss_type),
           'hp': np.array([HG.HEAD_HP['lr'], HG.HEAD_HP['betas'][0], HG.HEAD_HP['betas'][1], HG.HEAD_HP['eps'], HG.HEAD_HP['weight_decay'], 0.999]),
           'head_names': np.array(names), 'n_syncbn': np.array(n_sync)}
    state0 = net.state_dict()
    for k in state0:
        if k.startswith('proj_t.1.'):
            out['before/' + k] = state0[k].detach().numpy().copy()
    for s in range(steps):
        image, sparse = frames(s)
        model.train(prepare=True)
        output_depth, embedding, reference = model.forward(image=image, sparse_depth=sparse, loss_type=loss_type)
        loss, info = model.compute_loss(input_rgb=image, output_depth=output_depth, validity_map=None, ground_truth=None,
                                        embedding=embedding, reference=reference, loss_type='prepare')
        opt.zero_grad()
        loss.backward()
        p = 's%d/' % s
        out[p + 'loss'] = np.array(float(loss))
        named = dict(net.named_parameters())
        for k in names:
            g = named[k].grad
            out[p + 'has_grad/' + k] = np.array(g is not None)
            if g is not None:
                put(out, p + 'grad/' + k, g.detach().numpy())
        opt.step()
        state = net.state_dict()
        for k in state:
            if k.startswith(('proj', 'pred')):
                put(out, p + 'after/' + k, state[k].detach().numpy())
        for k in names if s == steps - 1 else ():                       # both Adam moments after the last step
            st = opt.state.get(named[k], {})
            if 'exp_avg' in st:
                put(out, p + 'exp_avg/' + k, st['exp_avg'].numpy())
                put(out, p + 'exp_avg_sq/' + k, st['exp_avg_sq'].numpy())
        print(name, s, float(loss), 'syncbn modules', n_sync, flush=True)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, path


def nlspn_cases():
    import make_golden_nlspn as MN
    ema = MN.import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from proxytta import synth
    for name, loss_type, h, w, n, steps in CASES['nlspn']:
        model = ema.ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, offset=True, device=torch.device('cpu'))
        model._prepare_head(HG.PREPARE)

        def frames(s, h=h, w=w, n=n):
            raw, image1, sparse = MN.nlspn_frame(s, h, w, n)
            return torch.from_numpy(image1), torch.from_numpy(sparse)
        run_case(model, model.model.model, synth.formula_state_dict_nlspn(HG.PREPARE), frames, name, loss_type, steps, [h, w, n, steps], HG.put)


def costdcnet_cases():
    import make_golden_costdcnet as MC
    ema, _ = MC.MG.import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from proxytta import synth
    for name, loss_type, h, w, n, steps in CASES['costdcnet']:
        model = ema.ExternalModel_Adapt('costdcnet', 0.1, MC.MAX_DEPTH, max_input_depth=None, device=torch.device('cpu'))
        model._prepare_head(HG.PREPARE)

        def frames(s, h=h, w=w, n=n):
            raw, image1, sparse = MC.costdc_frame(s, h, w, n, 0.05)
            return torch.from_numpy(image1), torch.from_numpy(sparse)
        run_case(model, model.model.model, synth.formula_state_dict_costdcnet(HG.PREPARE), frames, name, loss_type, steps, [h, w, n, steps], HG.put)


def msg_chn_cases():
    import make_golden_head as MH
    ema, _ = MH.MG.import_reference()
    torch.manual_seed(0)
    for name, loss_type, h, w, n, steps in CASES['msg_chn']:
        model = ema.ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cpu'))
        model._prepare_head(MH.PREPARE_MODE)

        def frames(s, h=h, w=w, n=n):
            image, sparse = MH.synth.synthetic_frame(s, h, w, n)
            return torch.from_numpy(image), torch.from_numpy(sparse)
        run_case(model, model.model.model, MH.synth.formula_state_dict(MH.PREPARE_MODE, 1.0), frames, name, loss_type, steps, [h, w, n, steps], HG.put)


if __name__ == '__main__':
    which = sys.argv[1:] or ['nlspn', 'costdcnet', 'msg_chn']
    if len(which) > 1:          # each backbone's import shims want their own interpreter
        import subprocess
        raise SystemExit(max(subprocess.call([sys.executable, os.path.abspath(__file__), b]) for b in which))
    {'nlspn': nlspn_cases, 'costdcnet': costdcnet_cases, 'msg_chn': msg_chn_cases}[which[0]]()
