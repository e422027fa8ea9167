"""Shared by tests/golden/make_golden_costdc_source.py and tests/test_gpu_costdc_source.py: the weights and the cases of the CostDCNet
source-model fixtures.

The source model is the loaded checkpoint before any adaptation: every BatchNorm (15 BatchNorm2d of Encoder2D, 28 BatchNorm3d of the UNet3D,
the sparse encoder's nine) normalises with its LOADED running statistics in the scored forward.  The formula weights of proxytta.synth carry
near-trivial buffers, against which an engine that normalised with zeros and ones would nearly pass.  Here gamma is 0.6 .. 0.85 or
1.15 .. 1.4 and beta +-0.2 (deterministic functions of the tensor's name), and the running statistics are what a trained checkpoint would
hold -- the statistics of the network's own activations on frame 0 at 64 x 96, measured by the generator on the reference -- moved away per
channel (tests/nlspn_meta_cases.perturb_stats: the mean by up to +-0.3 standard deviations, the variance by a factor 1.1 .. 1.5 up or
down).  They are stored once, in costdc_source_64x96.npz (`bn/<name>`)."""
import os

import numpy as np

from proxytta import synth
from tests.nlspn_meta_cases import perturb_stats

PREPARE = 'meta_selfsup_seq_1layer_ema'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MAX_DEPTH = 8.0
# (fixture, height, width, frames): 72 x 100 takes the dual-corner padding (the network batch doubles)
SOURCE_EVAL = [('costdc_source_64x96', 64, 96, 1), ('costdc_source_72x100_pad', 72, 100, 1), ('costdc_source_64x64_n2', 64, 64, 2)]
BASELINE_FIRST = [('costdc_bnadapt_64x96', 64, 96, 1), ('costdc_bnadapt_64x64_n2', 64, 64, 2)]      # one step each
BASELINE_SEQ = ('costdc_bnadapt_64x96_seq6', 64, 96, 1)                                             # six frames, one parameter set
STAGE3_ONLY =('conv1_rgb_meta.', 'proj', 'pred')          # what _prepare_head adds: a stage-3 checkpoint holds them, `_forward` runs none


def canonical(prefix):
    """ResBlock.norm3 is registered a second time as downsample[1] (one module, two names): one set of values for both."""
    return prefix[:-len('downsample.1')] + 'norm3' if prefix.startswith('enc2d.') and prefix.endswith('.downsample.1') else prefix


def bn_prefixes(sd):
    return [k[:-len('.running_mean')] for k in sd if k.endswith('.running_mean')]


def source_state_dict(stats=None, stage3=False):
    """The fixtures' checkpoint.  stats: {'<prefix>.running_mean' / '.running_var': array} by canonical prefix; None reads them from
    costdc_source_64x96.npz.  stage3: keep the meta conv and the heads, as a checkpoint saved after stage 2 does."""
    sd = synth.formula_state_dict_costdcnet(PREPARE)
    if not stage3:
        sd = {k: v for k, v in sd.items() if not k.startswith(STAGE3_ONLY)}
    if stats is None:
        with np.load(os.path.join(GOLDEN, 'costdc_source_64x96.npz')) as z:
            stats = {k[3:]: z[k] for k in z.files if k.startswith('bn/')}
    for pre in bn_prefixes(sd):
        if pre.startswith(STAGE3_ONLY):
            continue
        can = canonical(pre)
        n = sd[pre + '.weight'].shape[0]
        u = [synth.hash_uniform(can + '#src%d' % j, n) for j in (2, 3, 4)]
        g = 0.15 + 0.25 * u[0]
        sd[pre + '.weight'] = np.where(u[1] < 0.5, 1.0 - g, 1.0 + g).astype(np.float32)
        sd[pre + '.bias'] = (0.4 * u[2] - 0.2).astype(np.float32)
        for leaf in ('.running_mean', '.running_var'):
            if can + leaf in stats:
                sd[pre + leaf] = np.asarray(stats[can + leaf], dtype=np.float32)
    return sd


def baseline_names():
    """adapt_parameters('meta_bn') on the unprepared model: gamma / beta of Encoder2D's 15 BatchNorm2d in module order (norm3 once)."""
    out = []
    for k in synth.formula_state_dict_costdcnet(PREPARE):
        if k.startswith('enc2d.') and k.endswith('.running_mean') and '.downsample.1.' not in k:
            out += [k[:-len('running_mean')] + 'weight', k[:-len('running_mean')] + 'bias']
    return out


def moved_stats(pre, mean, var):
    return perturb_stats(pre, mean, var)
