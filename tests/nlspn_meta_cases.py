"""Shared by tests/golden/make_golden_nlspn_meta.py and tests/test_gpu_nlspn_meta.py: the weights of the adapt_mode 'meta' fixtures.

'meta' (src/nlspn_model_adapt.py:302-311) keeps every BatchNorm2d's loaded running statistics and gamma / beta and evaluates from them in
the scored forward.  The formula weights of proxytta.synth carry near-trivial buffers (mean 0.1 u, var 1 + 0.2 |u|, gamma 1 + 0.1 u): an
engine that normalised with zeros and ones would nearly pass against them.  Here gamma is 0.6 .. 0.85 or 1.15 .. 1.4 and beta +-0.2,
deterministic functions of the tensor's name (synth.hash_uniform).  The running statistics cannot be drawn freely: 36 normalisations deep, a
network whose buffers are unrelated to its activations diverges (the reference's eval depth reached 8e4 with random buffers).  They are what a
trained checkpoint would hold -- the statistics of the network's own activations on frame 0, measured by the generator on the reference --
and then moved away from them, per channel: the mean by up to +-0.3 standard deviations, the variance by a factor 1.1 .. 1.5 up or down.  So
they equal neither (0, 1) nor the batch statistics of any frame.  They are stored once, in nlspn_meta_32x64.npz (`bn/<name>`)."""
import os

import numpy as np

from proxytta import synth

PREPARE = 'meta_selfsup_seq_1layer_ema'
META_NAMES = ['conv1_rgb_meta.weight', 'conv1_rgb_meta.bias']           # the reference's adapt_parameters('meta') list, in order
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def is_bn2d(prefix):
    """BatchNorm2d modules of the backbone; the heads' proj / proj_t / pred hold BatchNorm1d, which 'meta' leaves alone."""
    return not prefix.startswith(('proj', 'pred'))


def bn2d_prefixes(sd):
    return [k[:-len('.running_mean')] for k in sd if k.endswith('.running_mean') and is_bn2d(k)]


def perturb_stats(pre, mean, var):
    """Measured (mean, var) of one BatchNorm2d -> the buffers the fixtures load."""
    n = mean.shape[0]
    u = [synth.hash_uniform(pre + '#meta%d' % j, n) for j in (0, 1)]
    f = np.exp(np.where(u[1] < 0.5, -1.0, 1.0) * (np.log(1.1) + np.abs(2.0 * u[1] - 1.0) * (np.log(1.5) - np.log(1.1))))
    return (mean + 0.6 * (u[0] - 0.5) * np.sqrt(var)).astype(np.float32), (var * f).astype(np.float32)


def meta_state_dict(stats=None):
    """stats: {'<prefix>.running_mean' / '.running_var': array}; None reads them from nlspn_meta_32x64.npz."""
    sd = synth.formula_state_dict_nlspn(PREPARE)
    if stats is None:
        with np.load(os.path.join(GOLDEN, 'nlspn_meta_32x64.npz')) as z:
            stats = {k[3:]: z[k] for k in z.files if k.startswith('bn/')}
    for pre in bn2d_prefixes(sd):
        n = sd[pre + '.weight'].shape[0]
        u = [synth.hash_uniform(pre + '#meta%d' % j, n) for j in (2, 3, 4)]
        g = 0.15 + 0.25 * u[0]
        sd[pre + '.weight'] = np.where(u[1] < 0.5, 1.0 - g, 1.0 + g).astype(np.float32)
        sd[pre + '.bias'] = (0.4 * u[2] - 0.2).astype(np.float32)
        for leaf in ('.running_mean', '.running_var'):
            if pre + leaf in stats:
                sd[pre + leaf] = np.asarray(stats[pre + leaf], dtype=np.float32)
    return sd
