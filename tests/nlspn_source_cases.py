"""Shared by tests/golden/make_golden_nlspn_source.py and the NLSPN source-model / BatchNorm-baseline tests: the weights of those fixtures.

The network is NLSPN without `_prepare_head`: no conv1_rgb_meta, no heads (NLSPNModel_Adapt._forward, nlspnmodel_adapt.py:792-848).  gamma / beta
are those of tests/nlspn_meta_cases.py (far from (1, 0)); the running statistics are the SOURCE model's own activation statistics on frame 0,
measured by the generator on the reference and then moved away per channel with perturb_stats, as the adapt_mode 'meta' fixtures do.  They are
stored once, in nlspn_source_32x64.npz (`bn/<name>`)."""
import os

import numpy as np

from tests.nlspn_meta_cases import GOLDEN, bn2d_prefixes, meta_state_dict

NOT_IN_SOURCE = ('conv1_rgb_meta', 'proj', 'pred')         # what _prepare_head adds (proj, proj_t, pred, the meta layer)
SOURCE_EVAL = ('nlspn_source_32x64', 'nlspn_source_40x56_n2')
BASELINE_FIRST = ('nlspn_bnadapt_32x64', 'nlspn_bnadapt_40x56_n2')
BASELINE_SEQ = 'nlspn_bnadapt_32x64_seq6'


def source_stats():
    with np.load(os.path.join(GOLDEN, SOURCE_EVAL[0] + '.npz')) as z:
        return {k[3:]: z[k] for k in z.files if k.startswith('bn/')}


def source_state_dict(stats=None, with_head=False):
    """The source model's state dict (reference key order).  stats: {'<prefix>.running_mean' / '.running_var': array}; None reads them from
    nlspn_source_32x64.npz.  with_head: the stage-3 form of the same checkpoint, which also holds the meta layer and the heads."""
    sd = meta_state_dict(stats=source_stats() if stats is None else stats)
    return sd if with_head else {k: v for k, v in sd.items() if not k.startswith(NOT_IN_SOURCE)}


def baseline_names(sd=None):
    """adapt_parameters('meta_bn') on a model whose head was never prepared (src/nlspn_model_adapt.py:322-337): no parameter is called
    'meta', so the list is gamma / beta of every BatchNorm2d in module order -- the 88-entry list without the two meta tensors."""
    sd = source_state_dict(stats={}) if sd is None else sd
    return [pre + leaf for pre in bn2d_prefixes(sd) for leaf in ('.weight', '.bias')]
