"""Generate the 2layers meta-block vectors of NLSPN and CostDCNet by running the REAL reference (read-only at /root/reference)
on CPU.

The 2layers recipe (prepare_mode 'meta_selfsup_seq_2layers_ema') replaces the 1layer conv1_rgb_meta by Res_Conv: NLSPN
Res_Conv(48, 256) on rgb1 (external_src/NLSPN/src/model/nlspnmodel_adapt.py:37-45, :1376-1377), CostDCNet Res_Conv(16, 64) on
Encoder2D's output (external_src/costdcnet/CostDCNet_adapt.py:555-563, :501-502).  Nothing is restated here: the existing
generators' case functions run with their PREPARE set to the 2layers mode, and every fixture gets its own `*2l_` name.

adapt_parameters('meta_bn') lists the block's seven tensors first and its two BatchNorm2d's gamma / beta a second time in the
BatchNorm pass (src/nlspn_model_adapt.py:322-337, src/costdcnet_model_adapt.py:357-378); `adapted_names` of each fixture records that
list, duplicates included.

Usage:  python tests/golden/make_golden_2layers_generic.py [case ...]      (each backbone's shims run in an interpreter of their own)
"""
import os
import re
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tta-depth-completion_amd'))

PREPARE = 'meta_selfsup_seq_2layers_ema'
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sd=1.0, w_sm=2.0, w_cos=0.1, max_input_depth=80.0)


def _nlspn():
    import make_golden_nlspn as MN
    MN.PREPARE = PREPARE
    return MN


def _costdcnet():
    import make_golden_costdcnet as MC
    MC.PREPARE = PREPARE
    return MC


def nlspn_case(name):
    MN = _nlspn()
    sys.path.insert(0, HERE)
    ema = MN.import_reference()
    if name == 'nlspn2l_32x64':
        MN.run_case(ema, name, 32, 64, 1, 2, HP)
    elif name == 'nlspn2l_32x64_legacy':
        MN.run_case(ema, name, 32, 64, 1, 1, HP, offset=True)
    elif name == 'nlspn2l_40x56_n2_legacy':           # odd encoder sizes: decoder crops (nlspnmodel_adapt.py:474-490)
        MN.run_case(ema, name, 40, 56, 2, 2, dict(HP, lr=3e-4), offset=True)
    elif name == 'nlspn2l_352x1216_legacy':
        MN.HOLES['allow'] = True
        MN.run_case(ema, name, 352, 1216, 1, 1, dict(HP, lr=3e-4), offset=True, sampled=True)
    elif name == 'nlspn2l_96x320_legacy_seq8':        # ONE parameter set over 8 frames, scored after every step; + the reference's own floor
        MN.HOLES['allow'] = True
        MN.run_case(ema, name, 96, 320, 1, 8, dict(HP, lr=3e-4), offset=True, sampled=True, light=True, alt=True)
    else:
        raise KeyError(name)


def costdcnet_case(name):
    MC = _costdcnet()
    ema, _ = MC.MG.import_reference()
    if name == 'costdcnet2l_64x96':
        MC.run_case(ema, name, 64, 96, 1, 2)
    elif name == 'costdcnet2l_72x100_pad':            # dual-corner padding, odd pooled sizes
        MC.run_case(ema, name, 72, 100, 1, 1)
    elif name == 'costdcnet2l_480x640':
        MC.run_case(ema, name, 480, 640, 1, 1, density=1500.0 / (480 * 640), sampled=True)
    else:
        raise KeyError(name)


def head_case(name):
    """Stage-2 head trainer (src/head_main.py:259-276) on a 2layers network: make_golden_head_generic's run_case, its frames."""
    import make_golden_head_generic as MH
    MH.PREPARE = PREPARE
    from proxytta import synth
    if name == 'head_nlspn2l_forward_48x80_n2':
        MN = _nlspn()
        ema = MN.import_reference()
        h, w, n, steps = 48, 80, 2, 2
        model = ema.ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, offset=True, device=torch.device('cpu'))
        model._prepare_head(PREPARE)
        sd = synth.formula_state_dict_nlspn(PREPARE)

        def frames(s):
            raw, image1, sparse = MN.nlspn_frame(s, h, w, n)
            return torch.from_numpy(image1), torch.from_numpy(sparse)
    elif name == 'head_costdcnet2l_forward_64x96_n2':
        MC = _costdcnet()
        ema, _ = MC.MG.import_reference()
        h, w, n, steps = 64, 96, 2, 2
        model = ema.ExternalModel_Adapt('costdcnet', 0.1, MC.MAX_DEPTH, max_input_depth=None, device=torch.device('cpu'))
        model._prepare_head(PREPARE)
        sd = synth.formula_state_dict_costdcnet(PREPARE)

        def frames(s):
            raw, image1, sparse = MC.costdc_frame(s, h, w, n, 0.05)
            return torch.from_numpy(image1), torch.from_numpy(sparse)
    else:
        raise KeyError(name)
    MH.run_case(model, model.model.model, sd, frames, name, 'head_selfsup_seq_ema', steps, [h, w, n, steps])


LIMIT = 1 << 20          # every committed file stays within 1 MiB
WSAMP = 8192


def shrink(name):
    """NLSPN's block weights (256 x 48 x 3 x 3 = 110,592 values each) would make a fixture of several MB: their per-step gradient /
    parameter / Adam moment maps are kept at WSAMP evenly spaced flat indices (`wsamp_idx`) under `wsamp/<key>`; the per-entry
    norms (grad_norms / param_norms) still cover the whole tensors."""
    path = os.path.join(HERE, name + '.npz')
    z = dict(np.load(path))
    n_keys = len(z)
    if '_seq' in name:          # sequences: tensors of the first step only (the scored maps and loss terms stay for every step)
        for k in [k for k in z if re.match(r'(wsamp/)?s[1-9][0-9]*/(grad|param)/', k)]:
            del z[k]
    big = [k for k in z if 'conv1_meta' in k and z[k].size > 4 * WSAMP]
    if big:
        n = z[big[0]].size
        idx = np.linspace(0, n - 1, WSAMP).astype(np.int64)
        z['wsamp_idx'] = idx
        for k in big:
            assert z[k].size == n, k
            z['wsamp/' + k] = z.pop(k).reshape(-1)[idx]
    if big or len(z) != n_keys:
        np.savez_compressed(path, **z)
    size = os.path.getsize(path)
    print('fixture', path, size, 'bytes', flush=True)
    assert size <= LIMIT, '%s is %d bytes (limit %d)' % (path, size, LIMIT)


CASES = {
    'nlspn2l_32x64': nlspn_case, 'nlspn2l_32x64_legacy': nlspn_case, 'nlspn2l_40x56_n2_legacy': nlspn_case,
    'nlspn2l_352x1216_legacy': nlspn_case, 'nlspn2l_96x320_legacy_seq8': nlspn_case,
    'costdcnet2l_64x96': costdcnet_case, 'costdcnet2l_72x100_pad': costdcnet_case, 'costdcnet2l_480x640': costdcnet_case,
    'head_nlspn2l_forward_48x80_n2': head_case, 'head_costdcnet2l_forward_64x96_n2': head_case,
}

if __name__ == '__main__':
    which = sys.argv[1:] or list(CASES)
    if len(which) > 1:
        for c in which:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), c])
            if rc:
                raise SystemExit(rc)
        raise SystemExit(0)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    CASES[which[0]](which[0])
    shrink(which[0])
