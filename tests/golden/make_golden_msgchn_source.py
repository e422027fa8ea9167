"""Generate the MSG_CHN source-model golden vectors by running the REAL reference on the CPU (where make_golden.py finds it).

The shims are make_golden.py's (imported from it: the reference is imported in place, nothing of it is copied); frames and weights come from
proxytta.synth through tests/msgchn_source_cases.py.  What differs is the driven network: ExternalModel_Adapt('msg_chn') WITHOUT
`_prepare_head`, whose forward with loss_type 'pretrain' (the reference's default) is `network._forward`
(network_exp_msg_chn_adapt.py:402-403, :418-461): no conv1_rgb_meta, no zero-image pass, no heads.  In eval mode the adapter returns its
first scale, `output_d11`, alone (src/msg_chn_model_adapt.py:179-181), after the dual-corner padding and the mean of the two crops for sizes
not divisible by 16 (:131-199).
Asserted here, on the CPU:
  * the unprepared model's state-dict keys are the formula checkpoint's minus conv1_rgb_meta.* / proj* / pred*;
  * a PREPARED 1layer model holding the same backbone tensors, called with 'pretrain', returns the unprepared model's depth bit for bit
    (stored as its own vector all the same);
  * the same weights' 'meta_selfsup_seq_ema' eval depth, with the fixtures' meta convolution, is more than 1e-2 relative MAE from the source
    depth (`tta_eval_rel_mae`): otherwise the fixtures could not tell the two networks apart;
  * the eval forward writes no tensor of the model.
Usage:  python tests/golden/make_golden_msgchn_source.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tta-depth-completion_amd'))
import make_golden as G  # noqa: E402
from tests.msgchn_source_cases import MAX_INPUT_DEPTH, ONE, PREPARED, SOURCE_EVAL, STAGE3_ONLY, frame, source_state_dict  # noqa: E402

EVAL_TYPE = 'pretrain'                       # the reference's default loss_type
TTA_EVAL_TYPE = 'meta_selfsup_seq_ema'       # the ProxyTTA network's eval forward


def rel_mae(a, b):
    return float((a - b).abs().mean() / b.abs().mean())


def model_of(ema, prepare_mode=None):
    model = ema.ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=MAX_INPUT_DEPTH, device=torch.device('cpu'))
    if prepare_mode is not None:
        model._prepare_head(prepare_mode)
    net = model.model.model
    sd = source_state_dict(prepare_mode)
    assert list(sd.keys()) == list(net.state_dict().keys()), 'key table drifted from reference'
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.eval()
    return model, net


def eval_depth(model, net, h, w, n, loss_type):
    image_np, sparse_np = frame(h, w, n)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        depth = model.forward(image=torch.from_numpy(image_np), sparse_depth=torch.from_numpy(sparse_np), loss_type=loss_type)
    now = net.state_dict()
    assert list(now.keys()) == list(before.keys()) and all(torch.equal(v, now[k]) for k, v in before.items()), 'the eval forward wrote a tensor'
    assert tuple(depth.shape) == (n, 1, h, w)
    return depth


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ema, _ = G.import_reference()
    source, snet = model_of(ema)
    assert not [k for k in snet.state_dict() if k.startswith(STAGE3_ONLY)]
    prepared, pnet = model_of(ema, ONE)
    assert all(torch.equal(v, pnet.state_dict()[k]) for k, v in snet.state_dict().items())         # the same backbone tensors
    for name, h, w, n in SOURCE_EVAL:
        depth = eval_depth(source, snet, h, w, n, EVAL_TYPE)
        again = eval_depth(prepared, pnet, h, w, n, EVAL_TYPE)
        assert torch.equal(depth, again), 'a prepared model\'s \'pretrain\' is not the unprepared model\'s'
        tta = eval_depth(prepared, pnet, h, w, n, TTA_EVAL_TYPE)
        apart = rel_mae(tta, depth)
        assert apart > 1e-2, apart
        out = {'meta': np.array([h, w, n, 0], dtype=np.int64), 'max_input_depth': np.array(MAX_INPUT_DEPTH), 'depth_eval': depth.numpy(),
               'tta_eval_rel_mae': np.array(apart)}
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
        print('%s: depth mean %.4f min %.4f max %.4f; the ProxyTTA eval depth is %.3e away' % (name, float(depth.mean()), float(depth.min()),
              float(depth.max()), apart), flush=True)
        if (h, w, n) == (32, 48, 1):
            np.savez_compressed(os.path.join(HERE, PREPARED + '.npz'), **dict(out, depth_eval=again.numpy()))
