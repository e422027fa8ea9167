"""ExternalModel_Adapt.adapt(..., augmenter=...) against the reference's inner loop written by hand with the calls the project already
has (src/tta_main.py:579-633: geo.transform, pho.transform, step, then the eval forward): everything bit-identical, the random state too."""
import numpy as np
import pytest
import torch

from proxytta import synth
from proxytta.augment import StepAugmenter
from proxytta.model import CANONICAL_LOSS_TYPE, ExternalModel_Adapt
from proxytta.transforms import Transforms
from tests.util import ONE

pytestmark = pytest.mark.gpu

MODES = ['bilinear', 'nearest', 'nearest', 'nearest']
H, W = 64, 96
SEED = 3


def make_msgchn():
    """tests/test_gpu_score.py::make_model, taking the raw 0..255 image the photometric jitter works on"""
    model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
    model._prepare_head(ONE)
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict(ONE).items()})
    opt = torch.optim.Adam(model.adapt_parameters(mode='meta'), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
    model.model.bind_optimizer(opt)
    model.set_image_norm([0, 1])
    return model, opt


def make_costdcnet():
    model = ExternalModel_Adapt('costdcnet', 0.1, 8.0, max_input_depth=None, device=torch.device('cuda'))
    model._prepare_head(ONE)
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict_costdcnet().items()})
    opt = torch.optim.Adam(model.adapt_parameters(mode='meta_bn'), lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
    model.model.bind_optimizer(opt)
    model.set_image_norm([[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]])
    return model, opt


def frame(idx, n, **kw):
    image01, sparse = synth.synthetic_frame(idx, H, W, n, **kw)
    image = torch.from_numpy(np.floor(image01 * 255.0).astype(np.float32)).cuda()
    sparse = torch.from_numpy(sparse).cuda()
    gt = torch.from_numpy(synth.synthetic_frame(idx + 100, H, W, n, density=1.0, **{k: v for k, v in kw.items() if k != 'density'})[1]).cuda()
    return image, sparse, torch.where(sparse > 0, torch.ones_like(sparse), sparse), gt


def vkitti():
    """bash/adapt/adapt_msgchn_vkitti.sh:34-41"""
    return (Transforms(random_flip_type=['horizontal'], random_rotate_max=5, random_resize_and_crop=[1.0, 1.5]),
            Transforms(random_brightness=[0.6, 1.4], random_contrast=[0.6, 1.4], random_saturation=[0.6, 1.4]))


def by_hand(model, geo, pho, image, sparse, valid, gt, inner_iter, probability, drawn):
    model.train()
    info = None
    for _ in range(inner_iter):
        im, sp, vm, _gt = geo.transform([image, sparse, valid, gt], interpolation_modes=MODES, random_transform_probability=probability)
        [im1] = pho.transform([im], random_transform_probability=probability)
        drawn.append((geo.last_draw, pho.last_draw))
        info, _ = model.step(im1, sp, vm, loss_image=im)
    model.eval()
    return model.forward(image, sparse, loss_type=CANONICAL_LOSS_TYPE), info


def seed_all():
    torch.manual_seed(SEED)
    np.random.seed(SEED)


def rng_state():
    s = np.random.get_state()
    return torch.get_rng_state(), (s[0], s[1].tolist(), s[2], s[3], s[4])


def adam_state(model, opt, mode):
    out = []
    for p in model.adapt_parameters(mode=mode):
        st = opt.state[p]
        out += [p.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone(), torch.as_tensor(float(st['step']))]
    return out


def run_both(make, mode, transforms, n, inner_iter, n_frames, **frame_kw):
    ours, opt_a = make()
    hand, opt_b = make()
    frames = [frame(i, n, **frame_kw) for i in range(n_frames)]
    seed_all()
    aug = StepAugmenter(*transforms(), MODES)
    drawn_a, routes = [], []
    draw, apply = aug.draw, aug.apply
    aug.draw = lambda *a, **k: drawn_a.append(draw(*a, **k)) or drawn_a[-1]
    aug.apply = lambda *a, **k: (apply(*a, **k), routes.append(aug.path))[0]
    got = [ours.adapt(image, sparse, inner_iter=inner_iter, validity_map=valid, augmenter=aug, augmentation_probability=1.0)
           for image, sparse, valid, gt in frames]
    got = [(d.clone(), i.clone()) for d, i in got]
    state_a = rng_state()
    seed_all()
    geo, pho = transforms()
    drawn_b = []
    want = [by_hand(hand, geo, pho, image, sparse, valid, gt, inner_iter, 1.0, drawn_b) for image, sparse, valid, gt in frames]
    state_b = rng_state()
    torch.cuda.synchronize()
    assert len(drawn_a) == len(drawn_b) == inner_iter * n_frames and routes == ['fused'] * len(drawn_a)
    for (da, ia), (db, ib) in zip(got, want):
        assert torch.isfinite(da).all() and torch.equal(da, db) and torch.equal(ia, ib)
    for a, b in zip(adam_state(ours, opt_a, mode), adam_state(hand, opt_b, mode)):
        assert torch.equal(a, b)
    assert torch.equal(state_a[0], state_b[0]) and state_a[1] == state_b[1]
    return drawn_a, ours


def test_msgchn_adapt_equals_the_loop_by_hand():
    """MSG_CHN, 64 x 96, N = 2, inner_iter = 3, the vkitti flags at probability 1.0, two frames."""
    drawn, model = run_both(make_msgchn, 'meta', vkitti, 2, 3, 2)
    assert any(bool(g['rotate'][0].any()) for g, _ in drawn) and any(bool(g['resize'][0].any()) for g, _ in drawn)      # SEED is chosen so
    assert any(bool(g['hflip'].any()) for g, _ in drawn) and any(bool(p['contrast'][0].any()) for _, p in drawn)
    assert int(model.model._adam_t) == 6


def test_costdcnet_adapt_equals_the_loop_by_hand():
    """CostDCNet, N = 1, inner_iter = 1, flip and rotation only (bash/adapt/adapt_costdc_scannet.sh), a photometric object with nothing configured."""
    flags = lambda: (Transforms(random_flip_type=['horizontal'], random_rotate_max=5), Transforms())
    drawn, _ = run_both(make_costdcnet, 'meta_bn', flags, 1, 1, 2, density=0.05, dmin=0.3, dmax=7.5)
    assert any(bool(g['rotate'][0].any()) for g, _ in drawn)


def test_without_an_augmenter_nothing_changes_and_the_two_refusals():
    image, sparse, valid, gt = frame(0, 2)
    plain, opt_a = make_msgchn()
    same, opt_b = make_msgchn()
    seed_all()
    before = rng_state()
    for _ in range(2):
        d0, i0 = plain.adapt(image, sparse, inner_iter=2, validity_map=valid)
        d1, i1 = same.adapt(image, sparse, inner_iter=2, validity_map=valid, augmenter=None, augmentation_probability=1.0, generator=torch.Generator())
        assert torch.equal(d0, d1) and torch.equal(i0, i1)
    for a, b in zip(adam_state(plain, opt_a, 'meta'), adam_state(same, opt_b, 'meta')):
        assert torch.equal(a, b)
    after = rng_state()
    assert torch.equal(before[0], after[0]) and before[1] == after[1]
    aug = StepAugmenter(*vkitti())
    with pytest.raises(ValueError, match='loss_image'):
        same.adapt(image, sparse, augmenter=aug, loss_image=image)
    with pytest.raises(ValueError, match='look-ahead prefix'):
        same.adapt(image, sparse, augmenter=aug, next_frame=(image, sparse))
    assert aug.last_draw is None                                                        # refused before anything was drawn


def test_probability_zero_is_the_frame_as_passed():
    image, sparse, valid, gt = frame(1, 2)
    aug = StepAugmenter(*vkitti())
    gen = torch.Generator().manual_seed(SEED)
    g, p = aug.draw(2, H, W, 0.0, gen)
    assert not any(bool(t.any()) for t in (g['hflip'], g['rotate'][0], g['resize'][0], p['brightness'][0], p['contrast'][0], p['saturation'][0]))
    image1, loss_image, sparse1, valid1, gt1 = aug.apply(image, sparse, valid, gt)
    assert aug.path == 'fused'
    assert torch.equal(sparse1, sparse) and torch.equal(loss_image, image) and torch.equal(valid1, valid) and torch.equal(gt1, gt)
    assert torch.equal(image1, image)                                                   # an integer-valued 0..255 image survives the truncation
