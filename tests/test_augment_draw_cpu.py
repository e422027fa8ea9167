"""The host side of the augmented inner loop (proxytta/augment.py), no GPU: StepAugmenter.draw consumes the random streams exactly as
the two Transforms.draw calls of src/tta_main.py:595-604 do, pack_draw writes include/ptta.h's ptta_augment_draw field by field, and
fused_eligible sends every draw the one-launch kernel does not cover to the staged calls."""
import os
import re

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.augment import DRAW_DTYPE, StepAugmenter, fused_eligible, pack_draw
from proxytta.transforms import Transforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('bilinear', 'nearest', 'nearest', 'nearest')


def vkitti(**more):
    """bash/adapt/adapt_msgchn_vkitti.sh:34-41"""
    geo = Transforms(random_flip_type=['horizontal'], random_rotate_max=5, random_resize_and_crop=[1.0, 1.5], **more)
    pho = Transforms(random_brightness=[0.6, 1.4], random_contrast=[0.6, 1.4], random_saturation=[0.6, 1.4])
    return geo, pho


def same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    return a is b if a is None else a == b


def empty_draw():
    return dict.fromkeys(('crop', 'hflip', 'vflip', 'rotate', 'resize', 'brightness', 'contrast', 'saturation', 'gamma', 'hue', 'noise', 'crop_pad',
                          'resize_pad', 'remove'))


@pytest.mark.parametrize('use_generator', [False, True])
@pytest.mark.parametrize('crop', [False, True])
def test_draw_consumes_the_streams_as_the_two_draws_do(use_generator, crop):
    n, h, w, p = 3, 40, 64, 0.8
    more = dict(random_crop_to_shape=[20, 24, 30, 40]) if crop else {}          # the range crop draws its size from numpy's global state

    def run(by_hand):
        gen = torch.Generator().manual_seed(11) if use_generator else None
        torch.manual_seed(5)
        np.random.seed(7)
        geo, pho = vkitti(**more)
        if by_hand:
            g = geo.draw(n, h, w, p, gen, channels=(3, 1, 1, 1))
            gh, gw = (g['crop'][0], g['crop'][1]) if g['crop'] is not None else (h, w)
            q = pho.draw(n, gh, gw, p, gen, channels=(3,))
        else:
            aug = StepAugmenter(geo, pho, MODES)
            g, q = aug.draw(n, h, w, p, gen)
            assert aug.last_draw == (g, q) and geo.last_draw is g and pho.last_draw is q
        return g, q, torch.rand(1, generator=gen), torch.rand(1), np.random.rand()

    a, b = run(True), run(False)
    for da, db in zip(a[:2], b[:2]):
        assert da.keys() == db.keys()
        for key in da:
            assert same(da[key], db[key]), key
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[4] == b[4]
    assert a[0]['rotate'] is not None and a[0]['resize'] is not None and a[1]['contrast'] is not None and (a[0]['crop'] is not None) == crop


def test_draw_without_a_photometric_object():
    geo, _ = vkitti()
    aug = StepAugmenter(geo)
    torch.manual_seed(1)
    g, q = aug.draw(2, 16, 16, 1.0)
    assert q is None and g['hflip'] is not None and fused_eligible(g, q, aug.interpolation_modes)


def test_draw_record_mirrors_the_header():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    body = re.search(r'typedef struct ptta_augment_draw \{(.*?)\} ptta_augment_draw;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r'(uint32_t|int32_t|float)\s+([^;]+);', body):
        fields += [(name.strip(), {'uint32_t': '<u4', 'int32_t': '<i4', 'float': '<f4'}[ctype]) for name in names.split(',')]
    assert fields == [(name, DRAW_DTYPE[name].str) for name in DRAW_DTYPE.names] and DRAW_DTYPE.itemsize == 52
    assert [DRAW_DTYPE.fields[name][1] for name in DRAW_DTYPE.names] == list(range(0, 52, 4))                 # packed, in order
    flags = dict(re.findall(r'(PTTA_AUG_[A-Z]+) = (\d+)', header))
    assert {k: int(v) for k, v in flags.items()} == {k: getattr(_lib, k) for k in dir(_lib) if k.startswith('PTTA_AUG_')} and len(flags) == 9
    names = [n for n, _ in _lib.AugmentArgs._fields_]
    struct = re.search(r'typedef struct ptta_augment_args \{(.*?)\} ptta_augment_args;', header, re.S).group(1)
    struct = re.sub(r'/\*.*?\*/', '', struct, flags=re.S)
    declared = [x.strip().lstrip('*') for decl in re.findall(r'(?:const\s+)?[a-z_0-9]+\*?\s+([^;]+);', struct) for x in decl.split(',')]
    assert declared == names


def test_pack_draw_field_by_field():
    u8 = lambda *v: torch.tensor(v, dtype=torch.uint8)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    g = empty_draw()
    g.update(crop=(24, 40, i32(0, 16, 7), i32(24, 0, 3)), hflip=u8(1, 0, 1), vflip=u8(0, 0, 1),
             rotate=(u8(0, 1, 1), torch.tensor([0.1, -5.0, 33.0], dtype=torch.float64)),
             resize=(u8(1, 0, 1), i32(24, 30, 36), i32(40, 50, 60), i32(0, 3, 12), i32(0, 5, 20), 24, 40))
    q = empty_draw()
    q.update(brightness=(u8(1, 1, 0), torch.tensor([0.6, 1.4, 1.0])), contrast=(u8(0, 1, 0), torch.tensor([0.7, 1.3, 0.9])),
             gamma=(u8(0, 0, 1), torch.tensor([0.8, 1.2, 1.1])), hue=(u8(1, 0, 0), torch.tensor([-0.5, 0.5, 0.25])),
             saturation=(u8(0, 0, 1), torch.tensor([0.65, 1.35, 1.05])))
    r = pack_draw(g, q, 3)
    assert r.dtype == DRAW_DTYPE and r.shape == (3,)
    L = _lib
    assert r['flags'].tolist() == [L.PTTA_AUG_HFLIP | L.PTTA_AUG_RESIZE | L.PTTA_AUG_BRIGHTNESS | L.PTTA_AUG_HUE,
                                   L.PTTA_AUG_ROTATE | L.PTTA_AUG_BRIGHTNESS | L.PTTA_AUG_CONTRAST,
                                   L.PTTA_AUG_HFLIP | L.PTTA_AUG_VFLIP | L.PTTA_AUG_ROTATE | L.PTTA_AUG_RESIZE | L.PTTA_AUG_GAMMA | L.PTTA_AUG_SATURATION]
    assert r['crop_y'].tolist() == [0, 16, 7] and r['crop_x'].tolist() == [24, 0, 3]
    assert r['angle_deg'].tolist() == [float(np.float32(0.1)), -5.0, 33.0]             # the .float() of the float64 draw
    assert r['resize_height'].tolist() == [24, 30, 36] and r['resize_width'].tolist() == [40, 50, 60]          # a coin at 0 keeps its values
    assert r['resize_y'].tolist() == [0, 3, 12] and r['resize_x'].tolist() == [0, 5, 20]
    for key in ('brightness', 'contrast', 'gamma', 'hue', 'saturation'):
        assert r[key].tolist() == q[key][1].tolist(), key
    # nothing configured, no photometric draw: all zero; and `out` is overwritten entirely
    out = np.full(3, np.array((7,) * 13, dtype=DRAW_DTYPE), dtype=DRAW_DTYPE)
    z = pack_draw(empty_draw(), None, 3, out=out)
    assert z is out and z.tobytes() == bytes(3 * 52)
    # configured but every coin at 0: values kept, flags clear
    g0 = empty_draw()
    g0.update(hflip=u8(0, 0), rotate=(u8(0, 0), torch.tensor([1.5, -2.5], dtype=torch.float64)), resize=(u8(0, 0), i32(9, 9), i32(8, 8), i32(1, 2), i32(3, 4), 8, 8))
    q0 = empty_draw()
    q0.update(contrast=(u8(0, 0), torch.tensor([0.75, 1.25])))
    r0 = pack_draw(g0, q0, 2)
    assert r0['flags'].tolist() == [0, 0] and r0['angle_deg'].tolist() == [1.5, -2.5] and r0['resize_x'].tolist() == [3, 4]
    assert r0['contrast'].tolist() == [0.75, 1.25] and r0['brightness'].tolist() == [0.0, 0.0] and r0['crop_y'].tolist() == [0, 0]


def test_fused_eligible():
    u8 = torch.ones(2, dtype=torch.uint8)
    f = torch.ones(2)
    g, q = empty_draw(), empty_draw()
    assert fused_eligible(g, None, MODES) and fused_eligible(g, q, MODES)
    g.update(hflip=u8, rotate=(u8, f.double()), crop=(4, 4, u8.int(), u8.int()))
    q.update(brightness=(u8, f), gamma=(u8, f))
    assert fused_eligible(g, q, MODES) and fused_eligible(g, q, (2, 0, 0, 0)) and fused_eligible(g, q, ('nearest',) * 4)
    # what only the staged calls do
    for key, value in (('noise', (u8, [f])), ('crop_pad', (u8,) * 9), ('resize_pad', (u8,) * 7), ('remove', (u8, f, [[1, 1]] * 2))):
        assert not fused_eligible(dict(g, **{key: value}), q, MODES), key
        assert not fused_eligible(g, dict(q, **{key: value}), MODES), key
    # gamma as the only photometric option is the float branch
    only_gamma = dict(empty_draw(), gamma=(u8, f))
    assert not fused_eligible(g, only_gamma, MODES)
    assert fused_eligible(g, dict(only_gamma, hue=(u8, f * 0.1)), MODES)
    # fewer interpolation modes than tensors; a map that is not sampled nearest; a mode that is not built
    assert not fused_eligible(g, q, ('bilinear', 'nearest')) and not fused_eligible(g, q, ('bilinear',))
    assert not fused_eligible(g, q, ('bilinear', 'nearest', 'bilinear', 'nearest')) and not fused_eligible(g, q, ('bicubic', 'nearest', 'nearest', 'nearest'))
    # the two objects swapped: geometry in the photometric draw, jitter in the geometric one
    assert not fused_eligible(g, dict(q, hflip=u8), MODES) and not fused_eligible(dict(g, contrast=(u8, f)), q, MODES)
