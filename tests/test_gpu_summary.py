"""ptta_summary_compose / ptta_summary_image_flag (proxytta.summary) and ExternalModel_Adapt.log_summary on the GPU.  Every comparison is
torch.equal: against the REAL reference's grids (tests/golden/summary_*.npz, tables taken from the fixture: matplotlib is not needed here)
and against the numpy restatement (tests/summary_cases.py, itself held bit for bit to those fixtures by tests/test_summary_cpu.py).
Outputs are views inside buffers filled with a sentinel; the margins are checked after every call."""
import ctypes

import numpy as np
import pytest
import torch

from proxytta import _lib, summary
from proxytta.model import ExternalModel_Adapt
from tests import summary_cases as C

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0          # no fp32 result equals it (table entries and the images here are above -100)
SENTINEL_U8 = 0xA5
PAD = 64                     # elements on each side of a view: a view at PAD keeps the buffer's 16-byte alignment, PAD + 1 ... do not
IDS = [c['name'] for c in C.CASES]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def tables(golden_dir):
    """The fixture's colormap tables, on the host (numpy) and on the device; also registered, so that log_summary needs no matplotlib."""
    _, z = C.load_fixture(golden_dir, 'full_n1_list')
    host = {'viridis': z['viridis'], 'inferno': z['inferno']}
    for name, t in host.items():
        summary.register_colormap(name, t)
    return host, {k: dev(v) for k, v in host.items()}


class Guarded:
    """The grid as a view inside a sentinel-filled buffer"""

    def __init__(self, shape, dtype, pad=PAD):
        self.numel, self.pad = int(np.prod(shape)), pad
        self.fill = SENTINEL_U8 if dtype == torch.uint8 else SENTINEL
        self.buf = torch.full((pad + self.numel + PAD,), self.fill, dtype=dtype, device='cuda')
        self.out = self.buf[pad:pad + self.numel].view(shape)

    def margins_intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:self.pad] == self.fill).all()) and bool((self.buf[self.pad + self.numel:] == self.fill).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == self.fill).all())


def compose_checked(want, image_dtype, pad, **kw):
    """compose_grid into a guarded view of the expected grid's shape; the result equals `want` and the margins stand."""
    want = torch.from_numpy(np.ascontiguousarray(want))
    g = Guarded(tuple(want.shape), want.dtype, pad)
    got = summary.compose_grid(image_dtype=image_dtype, out=g.out, **kw)
    assert g.margins_intact()
    assert got.data_ptr() == g.out.data_ptr()
    assert torch.equal(got.cpu(), want), (image_dtype, pad, int((got.cpu() != want).sum()))


def check_both_forms(want_f32, pads=(PAD, PAD + 1, PAD + 2), **kw):
    """fp32 CHW and uint8 HWC, 16-byte-aligned and misaligned outputs (the 16-byte / 12-byte paths and the one-pixel paths)"""
    for pad in pads:
        compose_checked(want_f32, 'float32', pad, **kw)
        compose_checked(C.to_uint8_hwc(want_f32), 'uint8', pad, **kw)
    # and without `out`: the wrapper allocates the grid
    got = summary.compose_grid(image_dtype='float32', **kw)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want_f32)))


def grids_of(images, maps, rng_range, maxd, nips, tables_dev):
    """keyword arguments of the two compose calls of one log_summary: the image grid, the depth grid"""
    common = dict(max_predict_depth=maxd, normalized_image_range=rng_range, n_image_per_summary=nips, tables=tables_dev)
    d_images, d_maps = [dev(a) for a in images], {k: dev(v) for k, v in maps.items()}
    calls = []
    if images:
        calls.append(dict(common, image=d_images))
    if images or 'output_depth' in maps:
        calls.append(dict(common, image=d_images[-1:], **d_maps))
    return calls


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_fixture_grids(case, golden_dir, tables):
    """The library against the reference's own grids, both forms"""
    meta, z = C.load_fixture(golden_dir, case['name'])
    images = [z['image%d' % k] for k in range(len(case['images']))]
    maps = {k: z[k] for k in C.MAP_KEYS.values() if k in z}
    calls = grids_of(images, maps, meta['rng_range'], meta['maxd'], meta['nips'], tables[1])
    assert len(calls) == len(meta['image_tags'])
    for k, kw in enumerate(calls):
        check_both_forms(z['grid%d' % k], **kw)
        # the uint8 form is the writer's conversion of the reference's grid, in torch's own arithmetic
        want = (torch.from_numpy(z['grid%d' % k]) * 255).clip(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        assert torch.equal(summary.compose_grid(image_dtype='uint8', **kw).cpu(), want)


@pytest.mark.parametrize('entry', C.GENERATED, ids=[e[0] for e in C.GENERATED])
def test_generated_against_the_restatement(entry, tables):
    name, n, (h, w), nips, kinds, which = entry
    images, maps = C.generated_inputs(entry)
    for rng_range in (C.MEAN_STD, [0, 1]):
        want = C.restate_grid(images, maps, rng_range, 80.0, nips, tables[0])
        assert want.shape[1:] == C.grid_shape(min(n, nips), h, w, len(images) + sum(1 for k in ('output_depth', 'ground_truth') if k in maps) +
                                              int('sparse_depth' in maps and 'validity_map' in maps))
        kw = dict(max_predict_depth=80.0, normalized_image_range=rng_range, n_image_per_summary=nips, tables=tables[1],
                  image=[dev(a) for a in images], **{k: dev(v) for k, v in maps.items()})
        check_both_forms(want, pads=(PAD, PAD + 1, PAD + 2, PAD + 3), **kw)
        if not images:
            break


def test_image_flag_is_torch_max_above_10():
    rng = np.random.default_rng(5)

    def flag_of(t):
        f = summary.image_flag(t)
        assert f.dtype == torch.int32 and f.numel() == _lib.PTTA_SUMMARY_FLAG_WORDS
        got = int(f[0].item())
        assert got == int(bool(torch.max(t) > 10.0)), (tuple(t.shape), got)
        return got
    base = rng.random((2, 3, 5, 7)).astype(np.float32)
    assert flag_of(dev(base)) == 0
    for pos in (0, 1, 2, 3, 104, 207, 208, 209):                                       # the first and the last elements: the unaligned ends
        a = base.copy().reshape(-1)
        a[pos] = 10.0
        assert flag_of(dev(a).view(2, 3, 5, 7)) == 0                                   # exactly 10 is not above 10
        a[pos] = np.nextafter(np.float32(10), np.float32(11))
        assert flag_of(dev(a).view(2, 3, 5, 7)) == 1
        a[(pos + 50) % a.size] = np.nan
        assert flag_of(dev(a).view(2, 3, 5, 7)) == 0                                   # torch.max propagates NaN and NaN > 10 is false
        a[pos] = 0.5
        assert flag_of(dev(a).view(2, 3, 5, 7)) == 0
    a = base.copy()
    a[0, 0, 0, 0] = np.inf
    assert flag_of(dev(a)) == 1
    a[0, 0, 0, 0] = -np.inf
    assert flag_of(dev(a)) == 0
    # bases at every offset of a 16-byte line, and a tensor that takes every block of the first launch
    big = torch.zeros(1 * 3 * 9 * 11 + 8, device='cuda')
    for off in range(4):
        for pos in (0, 1, 2, 3, 296):
            big.zero_()
            view = big[off:off + 297].view(1, 3, 9, 11)
            assert flag_of(view) == 0
            big[off + pos] = 11.0
            assert flag_of(view) == 1
            big[off + pos] = 0.0
            if off:
                big[off - 1] = 99.0                                                    # outside the tensor: not read
            big[off + 297] = 99.0
            assert flag_of(view) == 0
    wide = torch.zeros(4, 3, 352, 1216, device='cuda')
    assert flag_of(wide) == 0
    wide[3, 2, 351, 1215] = 10.5
    assert flag_of(wide) == 1
    wide[1, 1, 100, 100] = float('nan')
    assert flag_of(wide) == 0


def test_refusals_leave_the_output_untouched(tables):
    entry = ('refusals', 2, (6, 8), 2, ('raw',), 'osvg')
    images, maps = C.generated_inputs(entry)
    img, (o, s, v, gt) = dev(images[0]), (dev(maps[k]) for k in C.MAP_KEYS.values())
    vir, inf = tables[1]['viridis'], tables[1]['inferno']
    gh, gw = C.grid_shape(2, 6, 8, 4)
    g = Guarded((3, gh, gw), torch.float32)
    flag = summary.image_flag(img)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    ALL = _lib.PTTA_SUMMARY_ROW_OUTPUT | _lib.PTTA_SUMMARY_ROW_SPARSE | _lib.PTTA_SUMMARY_ROW_GT

    def call(**kw):
        a = _lib.SummaryArgs()
        f = dict(n_show=2, height=6, width=8, n_images=1, rows=ALL, normalize=0, out_dtype=0, max_predict_depth=80.0, image0=img.data_ptr(),
                 flag0=flag.data_ptr(), output_depth=o.data_ptr(), sparse_depth=s.data_ptr(), validity_map=v.data_ptr(),
                 ground_truth=gt.data_ptr(), viridis=vir.data_ptr(), inferno=inf.data_ptr(), out=g.out.data_ptr())
        f.update(kw)
        a.image[0], a.image_div255[0] = f.pop('image0'), f.pop('flag0')
        for k, val in f.items():
            setattr(a, k, val)
        return lib.ptta_summary_compose(ctypes.byref(a), stream)
    refused = [dict(out=None), dict(n_images=0, rows=0), dict(image0=None), dict(n_images=-1), dict(n_images=_lib.PTTA_SUMMARY_MAX_IMAGES + 1),
               dict(output_depth=None), dict(sparse_depth=None), dict(validity_map=None), dict(ground_truth=None),
               dict(rows=_lib.PTTA_SUMMARY_ROW_SPARSE), dict(rows=_lib.PTTA_SUMMARY_ROW_GT), dict(rows=_lib.PTTA_SUMMARY_ROW_SPARSE | _lib.PTTA_SUMMARY_ROW_GT),
               dict(rows=8), dict(rows=ALL | 16), dict(out_dtype=2), dict(out_dtype=-1),
               dict(n_show=0), dict(n_show=-2), dict(height=0), dict(width=0), dict(height=-6), dict(width=-8),
               dict(height=2 ** 20, width=2 ** 10), dict(n_show=2 ** 20, height=2 ** 6, width=2 ** 4),
               dict(max_predict_depth=0.0), dict(max_predict_depth=-80.0), dict(max_predict_depth=float('inf')), dict(max_predict_depth=float('nan')),
               dict(viridis=None), dict(inferno=None), dict(rows=_lib.PTTA_SUMMARY_ROW_OUTPUT, viridis=None)]
    for kw in refused:
        assert call(**kw) == -22, kw
    assert lib.ptta_summary_compose(None, stream) == -22
    assert g.untouched()
    # what is not needed may be missing: no inferno table without an error map, no table at all for image rows
    assert call(rows=_lib.PTTA_SUMMARY_ROW_OUTPUT, inferno=None, sparse_depth=None, validity_map=None, ground_truth=None) == 0
    assert call(rows=0, viridis=None, inferno=None, output_depth=None) == 0
    # the same call, valid: it runs, and writes the reference's grid
    g = Guarded((3, gh, gw), torch.float32)                    # (`call` writes into the current `g`)
    assert call() == 0 and g.margins_intact()
    want = C.restate_grid(images, maps, None, 80.0, 2, tables[0])
    assert torch.equal(g.out.cpu(), torch.from_numpy(want))
    # ptta_summary_image_flag's own refusals
    fl = torch.full((_lib.PTTA_SUMMARY_FLAG_WORDS,), 77, dtype=torch.int32, device='cuda')
    for args in ((None, 10, fl.data_ptr()), (img.data_ptr(), 10, None), (img.data_ptr(), 0, fl.data_ptr()), (img.data_ptr(), -5, fl.data_ptr()),
                 (img.data_ptr() + 2, 10, fl.data_ptr()), (img.data_ptr(), 10, fl.data_ptr() + 1)):
        assert lib.ptta_summary_image_flag(args[0], args[1], args[2], stream) == -22, args
    torch.cuda.synchronize()
    assert bool((fl == 77).all())
    # through the wrapper
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        summary.compose_grid(max_predict_depth=80.0, tables=tables[1])                                       # no row at all
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        summary.compose_grid(output_depth=o, max_predict_depth=0.0, tables=tables[1])
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        summary.compose_grid(output_depth=o, max_predict_depth=80.0, n_image_per_summary=0, tables=tables[1])
    with pytest.raises(ValueError):
        summary.compose_grid(output_depth=o.cpu(), max_predict_depth=80.0, tables=tables[1])                 # no CPU fallback
    with pytest.raises(ValueError):
        summary.compose_grid(output_depth=o, sparse_depth=s[:1], validity_map=v, max_predict_depth=80.0, tables=tables[1])


class Recorder(object):
    def __init__(self):
        self.calls = []

    def add_image(self, tag, img, global_step=None, **kw):
        self.calls.append(('image', tag, global_step, img, kw))

    def add_scalar(self, tag, value, global_step=None):
        self.calls.append(('scalar', tag, global_step, value, {}))

    def add_histogram(self, tag, values, global_step=None):
        self.calls.append(('histogram', tag, global_step, values, {}))


@pytest.fixture(scope='module')
def facade():
    return ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))


@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_log_summary_end_to_end(case, where, golden_dir, tables, facade):
    """The calls a recording writer sees -- kinds, tags, order, steps, grids -- are the ones the reference's log_summary made"""
    meta, z = C.load_fixture(golden_dir, case['name'])
    put = (lambda a: torch.from_numpy(a.copy())) if where == 'host' else dev
    t_images = [put(z['image%d' % k]) for k in range(len(case['images']))]
    image = None if not t_images else (t_images if case['as_list'] else t_images[0])
    maps = {k: put(z[k]) for k in C.MAP_KEYS.values() if k in z}
    facade.max_predict_depth = meta['maxd']
    scalars = {k: (torch.tensor(v, device='cuda') if i % 2 == 0 else v) for i, (k, v) in enumerate(C.SCALARS.items())}        # our loss_info values are device tensors
    for image_dtype in ('float32', 'uint8'):
        rec = Recorder()
        facade.log_summary(rec, meta['tag'], meta['step'], image=image, normalized_image_range=meta['rng_range'], scalars=scalars,
                           n_image_per_summary=meta['nips'], image_dtype=image_dtype, **maps)
        assert all(c[2] == meta['step'] for c in rec.calls)
        # the reference's order: histograms, scalars, the image grid, the depth grid
        assert [(c[0], c[1]) for c in rec.calls] == ([('histogram', t) for t in meta['histogram_tags']] + [('scalar', t) for t in meta['scalar_tags']] +
                                                     [('image', t) for t in meta['image_tags']])
        hist = [c for c in rec.calls if c[0] == 'histogram']
        given = []
        if 'output_depth' in maps:
            given = [maps['output_depth']] + ([maps['sparse_depth']] if 'sparse_depth' in maps and 'validity_map' in maps else []) + \
                ([maps['ground_truth']] if 'ground_truth' in maps else [])
        assert len(hist) == len(given) and all(c[3] is t for c, t in zip(hist, given))          # the tensors as given
        assert [float(c[3]) for c in rec.calls if c[0] == 'scalar'] == meta['scalar_values']
        assert all(not torch.is_tensor(c[3]) or not c[3].is_cuda for c in rec.calls if c[0] == 'scalar')
        for k, c in enumerate(c for c in rec.calls if c[0] == 'image'):
            ref = torch.from_numpy(z['grid%d' % k])
            assert torch.is_tensor(c[3]) and not c[3].is_cuda
            if image_dtype == 'float32':
                assert c[4] == {} and c[3].dtype == torch.float32 and torch.equal(c[3], ref), c[1]
            else:
                assert c[4] == {'dataformats': 'HWC'} and c[3].dtype == torch.uint8
                assert torch.equal(c[3], (ref * 255).clip(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()), c[1]
    with pytest.raises(NotImplementedError):
        facade.log_summary(Recorder(), 'tag', 1, image=image, output_image=torch.zeros(1, 3, 4, 4))


def test_driver_call_patterns(tables, facade):
    """The two call sites of src/tta_main.py: after an adaptation step (:641-654: host tensors, a list of one image, n_image_per_summary 1,
    loss_info as scalars) and inside the validation forward (:738-751: device tensors, a plain image tensor, host floats as scalars)."""
    entry = ('driver', 2, (12, 20), 4, ('raw',), 'osvg')
    images, maps = C.generated_inputs(entry)
    rng_range = [0.485, 0.456, 0.406, 0.229, 0.224, 0.225]
    facade.max_predict_depth = 80.0
    info = torch.tensor([0.75, 0.5, 0.125, 0.0625], device='cuda')
    loss_info = {'loss': info[0], 'loss_smooth': info[1], 'loss_sparse_depth': info[2], 'loss_cos': info[3]}
    rec = Recorder()
    for step in (0, 5):                                                                  # "a reference-style loop"
        facade.log_summary(rec, tag='adapt', step=step, image=[torch.from_numpy(images[0])], sparse_depth=torch.from_numpy(maps['sparse_depth']),
                           output_depth=dev(maps['output_depth']).clone().detach().to(torch.device('cpu')),
                           validity_map=torch.from_numpy(maps['validity_map']), ground_truth=torch.from_numpy(maps['ground_truth']),
                           output_image=None, normalized_image_range=rng_range, scalars=loss_info, n_image_per_summary=1)
        facade.log_summary(summary_writer=rec, tag='eval-x', step=step, image=dev(images[0]), output_depth=dev(maps['output_depth']).clone().detach(),
                           sparse_depth=dev(maps['sparse_depth']), validity_map=dev(maps['validity_map']), ground_truth=dev(maps['ground_truth']),
                           normalized_image_range=rng_range, scalars={'mae': 1.5, 'rmse': 2.5, 'imae': 0.5, 'irmse': 0.25}, n_image_per_summary=4)
    per_step = 3 + 4 + 2
    assert len(rec.calls) == 4 * per_step
    for k, (tag, nips) in enumerate((('adapt', 1), ('eval-x', 4), ('adapt', 1), ('eval-x', 4))):
        calls = rec.calls[k * per_step:(k + 1) * per_step]
        want = C.restate_log_summary(tag, images, maps, rng_range, 80.0, nips, tables[0])
        got = [c for c in calls if c[0] == 'image']
        assert [c[1] for c in got] == [t for t, _ in want] == [tag + '_image', tag + '_image_output_sparse-error_groundtruth-error']
        for c, (_, grid) in zip(got, want):
            assert torch.equal(c[3], torch.from_numpy(grid)), c[1]
        assert all(c[2] == (0, 0, 5, 5)[k] for c in calls)
    assert [c[3] for c in rec.calls[3:7]] == [0.75, 0.5, 0.125, 0.0625]


def test_workload_size(tables):
    """352 x 1216 with N = 4, both forms, against the restatement; bit-identical from run to run"""
    name, n, (h, w), nips, kinds, which = C.FULL
    images, maps = C.generated_inputs(C.FULL)
    want = torch.from_numpy(C.restate_grid(images, maps, C.MEAN_STD, 80.0, nips, tables[0]))
    kw = dict(max_predict_depth=80.0, normalized_image_range=C.MEAN_STD, n_image_per_summary=nips, tables=tables[1],
              image=[dev(a) for a in images], **{k: dev(v) for k, v in maps.items()})
    assert tuple(want.shape) == (3, 4 * h + 4, 4 * (2 * w + 2) + 2)
    got = summary.compose_grid(image_dtype='float32', **kw)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(summary.compose_grid(image_dtype='float32', **kw), got)
    got8 = summary.compose_grid(image_dtype='uint8', **kw)
    assert torch.equal(got8.cpu(), (want * 255).clip(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous())
    assert torch.equal(summary.compose_grid(image_dtype='uint8', **kw), got8)
    one = summary.compose_grid(image_dtype='float32', **dict(kw, n_image_per_summary=1))
    assert torch.equal(one.cpu(), torch.from_numpy(C.restate_grid(images, maps, C.MEAN_STD, 80.0, 1, tables[0])))
