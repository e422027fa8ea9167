"""Shared by tests/golden/make_golden_msgchn_source.py, tests/test_msgchn_source_cpu.py and tests/test_gpu_msgchn_source.py: the cases and the
weights of the MSG_CHN source-model fixtures.

The source model is `network._forward` (network_exp_msg_chn_adapt.py:418-461): the loaded checkpoint without conv1_rgb_meta, without the
zero-image pass and without the heads.  MSG_CHN has no BatchNorm outside the heads and the 2layers meta block, so the weights are the formula
weights of proxytta.synth as they are; what tells the source model from the ProxyTTA network is the meta convolution alone, and the generator
asserts on the CPU that the two eval depths of the same weights are more than 1e-2 relative MAE apart."""
from proxytta import synth

ONE, TWO = 'meta_selfsup_seq_1layer_ema', 'meta_selfsup_seq_2layers_ema'
MAX_INPUT_DEPTH = 80.0
# (fixture, height, width, frames): the smallest sizes at which each form can go wrong -- one frame, a batch, and a size that takes the
# dual-corner padding (two network frames per image, mean of the two crops)
SOURCE_EVAL = [('msgchn_source_32x48', 32, 48, 1), ('msgchn_source_32x48_n2', 32, 48, 2), ('msgchn_source_36x52_pad', 36, 52, 1)]
PREPARED = 'msgchn_source_32x48_prepared'          # the same depth from a PREPARED 1layer model called with 'pretrain' (bit-equal, asserted)
STAGE3_ONLY = synth.MSG_CHN_STAGE3_ONLY


def source_state_dict(stage3=None):
    """The fixtures' checkpoint: stage 0 (None: the backbone alone) or the stage-3 form of prepare mode `stage3`, which adds the meta layer
    and the heads around the SAME backbone tensors."""
    return synth.formula_state_dict_source() if stage3 is None else synth.formula_state_dict(stage3)


def frame(h, w, n):
    return synth.synthetic_frame(0, h, w, n)
