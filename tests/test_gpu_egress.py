"""ptta_egress_raw (proxytta.egress.egress_raw) and RawFrameSink on the GPU: every comparison is exact, against the numpy restatement of
the reference's writers (tests/egress_cases.py, itself held bit for bit to what the real functions' files decode to by
tests/test_egress_cpu.py).  Every output is a view inside a larger byte buffer pre-filled with 0xA5, the output itself included, so an
element the kernel skipped shows; the guard bytes on both sides of the view are checked after every call."""
import os
import zlib

import numpy as np
import pytest
import torch

from proxytta import _lib, synth
from proxytta.egress import PLANES, egress_raw
from proxytta.ingest import ingest_raw
from proxytta.sink import RawFrameSink
from tests import egress_cases as C

pytestmark = pytest.mark.gpu
FILL = 0xA5
PAD = 256                    # guard bytes on each side of a view (a multiple of 16: pad = PAD keeps the buffer's alignment)
ONE = 'meta_selfsup_seq_1layer_ema'


def same(t, ref):
    """torch.equal of a device result and a numpy array, bit for bit (16-bit planes compared through their int16 view)"""
    t = t.cpu()
    r = torch.from_numpy(np.ascontiguousarray(ref).view(np.int16) if ref.dtype == np.uint16 else np.ascontiguousarray(ref))
    return t.shape == r.shape and torch.equal(t.view(torch.int16) if t.dtype == torch.uint16 else t, r)


class Guarded:
    """output planes as views inside 0xA5-filled byte buffers; pads[key] = bytes in front of the view (its alignment)"""

    def __init__(self, n, H, W, keys, pads=None):
        self.buf, self.out, self.pad, self.size = {}, {}, {}, {}
        for k in keys:
            pad = (pads or {}).get(k, PAD)
            size = n * H * W * (3 if k == 'image_u8' else 2)
            self.buf[k] = torch.full((pad + size + PAD,), FILL, dtype=torch.uint8, device='cuda')
            assert self.buf[k].data_ptr() % 16 == 0
            inner = self.buf[k][pad:pad + size]
            self.out[k] = inner.view(n, H, W, 3) if k == 'image_u8' else inner.view(torch.uint16).view(n, H, W)
            self.pad[k], self.size[k] = pad, size

    def margins_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:self.pad[k]] == FILL).all()) and bool((b[self.pad[k] + self.size[k]:] == FILL).all()) for k, b in self.buf.items())

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((b == FILL).all()) for b in self.buf.values())


def dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def start_dev(start):
    return None if start is None else tuple(torch.tensor(s, dtype=torch.int32).cuda() for s in start)


def check(depth, validity, image, dst_size, start, multiplier=256.0, image_scale=255.0, pads=None, to_dev=dev):
    """One call on guarded, pre-filled outputs: every plane equals the restatement and the guards stand."""
    first = [a for a in (depth, validity, image) if a is not None][0]
    n, (h, w) = first.shape[0], first.shape[2:]
    H, W = (h, w) if dst_size is None else dst_size
    ref = C.restate(depth, validity, image, dst_size, start, multiplier, image_scale)
    g = Guarded(n, H, W, list(ref), pads)
    got = egress_raw(to_dev(depth), to_dev(validity), to_dev(image), dst_size=dst_size, start=start_dev(start), multiplier=multiplier,
                     image_scale=image_scale, out=g.out)
    assert g.margins_intact()
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert got[k].data_ptr() == g.out[k].data_ptr()
        assert same(got[k], ref[k]), k
    return got


def pick(planes, combo):
    return [a if on else None for a, on in zip(planes, combo)]


@pytest.mark.parametrize('case', C.CASES, ids=[c[0] for c in C.CASES])
def test_case_table(case):
    name, n, dst_size, (h, w), start, _ = case
    planes = C.frames(zlib.crc32(name.encode()), n, h, w)
    for combo in C.COMBOS:
        check(*pick(planes, combo), dst_size, start)


def test_unaligned_bases():
    """Outputs whose first byte sits at every even offset of a 16-byte line (every offset of a word for the image), the two 16-bit planes
    on different offsets, and inputs one float off the 16-byte grid: the same results, the guards untouched."""
    planes = C.frames(78, 2, 5, 21)

    def shifted(a):
        if a is None:
            return None
        big = torch.zeros(a.size + 4, dtype=torch.float32, device='cuda')
        big[1:1 + a.size] = torch.from_numpy(a).cuda().flatten()
        return big[1:1 + a.size].view(a.shape)
    for off in range(8):
        pads = {'depth_u16': PAD + 2 * off, 'validity_u16': PAD + 2 * ((off + 3) % 8), 'image_u8': PAD + off}
        check(*planes, (7, 27), ([1, 2], [off, 6 - off]), pads=pads, to_dev=shifted if off % 2 else dev)
    check(*planes, None, None, pads={'depth_u16': PAD + 6, 'validity_u16': PAD + 10, 'image_u8': PAD + 1}, to_dev=shifted)


def test_values_the_reference_leaves_undefined():
    """Negative, -0 and NaN give 0; anything at or above the top of the range, +inf included, gives the top (include/ptta.h)."""
    odd = np.array([-1.0, -0.0, np.nan, -np.inf, np.inf, 3e38, 2.0 ** 31, 2.0 ** 31 / 256.0, 256.0, 255.998, 255.99609375, -1e-30, 1e-30, 0.0,
                    1.0 / 256.0, np.nextafter(np.float32(1.0 / 256.0), np.float32(0.0)), 70000.0, 1e10, -3e38, 0.5], dtype=np.float32)
    depth = np.resize(odd, (1, 1, 4, 20)).copy()
    validity = np.resize(odd[::-1], (1, 1, 4, 20)).copy()
    image = np.resize(np.concatenate([odd, odd / 255.0, [1.0, 1.004, 0.999999, 256.0 / 255.0]]).astype(np.float32), (1, 3, 4, 20)).copy()
    got = check(depth, validity, image, (5, 24), ([1], [3]))
    d = got['depth_u16'][0, 1, 3:23].cpu().numpy().tolist()
    assert d == [0, 0, 0, 0, 65535, 65535, 65535, 65535, 65535, 65535, 65535, 0, 0, 0, 1, 0, 65535, 65535, 0, 128]
    v = got['validity_u16'][0, 1, 3:23].cpu().numpy().tolist()          # the same values, reversed
    assert v == [256 if x > 0 else 0 for x in odd[::-1].tolist()] and v[17] == 0 and v[15] == 256          # NaN, +inf
    for mult, scale in ((1000.0, 1.0), (1.0, 3.5)):
        check(depth, validity, image, None, None, mult, scale)


def test_round_trips_with_ingest():
    """ingest(egress(z)) is the restated truncation divided by the multiplier, and egress(ingest(u16)) gives the 16-bit window back,
    both exactly, with the same starts and therefore the same window."""
    n, (H, W), (h, w), start = 2, (11, 37), (8, 24), ([2, 3], [5, 13])
    st = start_dev(start)
    depth = C.frames(31, n, h, w)[0]
    for mult in (256.0, 1000.0):
        stored = egress_raw(depth=dev(depth), dst_size=(H, W), start=st, multiplier=mult)['depth_u16']
        back = ingest_raw(sparse_u16=stored, size=(h, w), start=st, multiplier=mult)
        want = C.restate_depth(depth, mult).astype(np.float32) / np.float32(mult)
        assert same(back['sparse'], want) and same(back['validity'], (want > 0).astype(np.float32))
    rng = np.random.default_rng(32)
    u16 = (rng.integers(0, 65536, size=(n, H, W)) * (rng.random((n, H, W)) < 0.8)).astype(np.uint16)
    u16[0, 2, 5:9] = (0, 1, 65535, 65534)
    planes = ingest_raw(sparse_u16=torch.from_numpy(u16.view(np.int16)).cuda(), size=(h, w), start=st)
    again = egress_raw(depth=planes['sparse'], validity=planes['validity'], dst_size=(H, W), start=st)
    window = np.stack([u16[b, start[0][b]:start[0][b] + h, start[1][b]:start[1][b] + w] for b in range(n)])
    assert same(again['depth_u16'], C.paste(window, (H, W), start))
    assert same(again['validity_u16'], C.paste(np.where(window > 0, 256, 0).astype(np.uint16), (H, W), start))
    # all 65,536 values, and back
    every = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    z = ingest_raw(sparse_u16=torch.from_numpy(every.view(np.int16)).cuda())['sparse']
    assert same(egress_raw(depth=z)['depth_u16'], every)


@pytest.mark.parametrize('case', C.FULL, ids=[c[0] for c in C.FULL])
def test_full_size(case):
    name, n, dst_size, (h, w), start = case
    planes = C.frames(zlib.crc32(name.encode()), n, h, w)
    check(*planes, dst_size, start)
    check(planes[0], None, None, dst_size, start)


def test_two_runs_are_bit_identical():
    n, (H, W), (h, w), start = 2, (45, 131), (40, 120), start_dev(([3, 1], [7, 11]))
    planes = [dev(a) for a in C.frames(33, n, h, w)]
    a = egress_raw(*planes, dst_size=(H, W), start=start)
    b = egress_raw(*planes, dst_size=(H, W), start=start)
    for k in PLANES:
        assert a[k].data_ptr() != b[k].data_ptr() and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_refusals_leave_the_outputs_untouched():
    n, (H, W), (h, w) = 2, (6, 10), (4, 8)
    d, v, i = (dev(a) for a in C.frames(34, n, h, w))
    g = Guarded(n, H, W, PLANES)
    o = g.out
    refused = pytest.raises(RuntimeError, match=r'\(-22\): ptta_egress_raw')
    with refused:
        egress_raw(dst_size=(H, W), out=o)                                                                 # no input at all
    with refused:
        egress_raw(depth=d, dst_size=(H, W), out={'depth_u16': o['depth_u16'], 'image_u8': o['image_u8']})  # an output without its input
    with refused:
        egress_raw(depth=d, validity=v, dst_size=(H, W), out={'depth_u16': o['depth_u16']})                 # an input without its output
    with refused:
        egress_raw(d, v, i, dst_size=(h - 1, W))
    with refused:
        egress_raw(d, v, i, dst_size=(H, w - 1))
    for bad in (0.0, -256.0, float('inf'), float('nan')):
        with refused:
            egress_raw(d, v, i, dst_size=(H, W), multiplier=bad, out=o)
        with refused:
            egress_raw(d, v, i, dst_size=(H, W), image_scale=bad, out=o)
    lib = _lib.load()
    rc = lib.ptta_egress_raw(_lib.ptr(d), None, None, o['depth_u16'].data_ptr() + 1, None, None, n, h, w, H, W, None, None, 256.0, 255.0,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == -22 and b'2-byte aligned' in lib.ptta_last_error(None)
    # what the wrapper itself refuses
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        egress_raw(depth=d.cpu())
    with pytest.raises(TypeError):
        egress_raw(depth=d.double())
    with pytest.raises(TypeError):
        egress_raw(depth=d[:, :, :, ::2])
    with pytest.raises(ValueError):
        egress_raw(depth=d, validity=v[:, :, :3].contiguous())
    with pytest.raises(ValueError):
        egress_raw(depth=d, dst_size=(H, W), out={'depth_u16': o['depth_u16'][:1]})
    with pytest.raises(KeyError):
        egress_raw(depth=d, out={'depth': o['depth_u16']})
    assert g.untouched()
    egress_raw(d, v, i, dst_size=(H, W), out=o)                                                           # the same call, valid: it runs
    assert g.margins_intact() and same(o['depth_u16'], C.restate(d.cpu().numpy(), dst_size=(H, W))['depth_u16'])


# ---- host staging of the stored frames ----------------------------------------------------------------------
def test_sink_delivers_frames_in_order_while_the_source_is_overwritten():
    """Five frames through three slots.  The ONE device tensor every frame is submitted from is overwritten right behind each submit, as
    the engine overwrites its depth buffer in the next step: the collected planes still equal the direct call's, so the read is ordered
    on the caller's stream."""
    n, (H, W), (h, w) = 2, (45, 131), (40, 120)
    frames = [C.frames(200 + k, n, h, w) for k in range(5)]
    starts = [([k, 4 - k], [2 * k + 1, 9 - k]) for k in range(5)]
    sink = RawFrameSink(n, h, w, H, W, planes=('depth', 'validity', 'image'))
    assert sink.slots == 3 and sink.bytes_per_frame == sink.layout['bytes'] and sink.in_flight() == 0
    src = [torch.empty((n, c, h, w), dtype=torch.float32, device='cuda') for c in (1, 1, 3)]
    junk = [torch.full_like(t, float('nan')) for t in src]
    on_device = [[dev(a) for a in f] for f in frames]

    def submit(k):
        for t, a in zip(src, on_device[k]):
            t.copy_(a)
        sink.submit(*src, start=starts[k])
        for t, j in zip(src, junk):
            t.copy_(j)                                   # the next step's writes, enqueued right behind the submit
    seen = []
    for k in range(3):
        submit(k)
    assert sink.in_flight() == 3
    for k in range(5):
        got = sink.collect()
        seen.append(got['depth_u16'].ctypes.data)
        ref = C.restate(*frames[k], (H, W), starts[k])
        direct = egress_raw(*on_device[k], dst_size=(H, W), start=start_dev(starts[k]))
        for key in PLANES:
            assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (k, key)
            assert same(direct[key], got[key]), (k, key)
        sink.release()
        if k + 3 < 5:
            submit(k + 3)
    assert seen[:2] == seen[3:5] and len(set(seen)) == 3 and sink.in_flight() == 0
    # backpressure without a writer: collect() with nothing submitted and submit() with every slot unread both raise
    with pytest.raises(RuntimeError):
        sink.collect()
    with pytest.raises(RuntimeError):
        sink.release()
    for k in range(3):
        sink.submit(*on_device[k])
    with pytest.raises(RuntimeError, match='unread'):
        sink.submit(*on_device[3])
    sink.collect()
    with pytest.raises(RuntimeError):
        sink.collect()                                   # before release() of the collected one
    sink.release()
    sink.submit(*on_device[3])                           # one slot read: one submit goes through
    assert sink.in_flight() == 3
    with pytest.raises(ValueError):
        sink.submit(depth=on_device[0][0])               # not the planes the sink was built with
    with pytest.raises(ValueError):
        sink.submit(*on_device[0], paths=['a.png'] * n)  # paths without a writer
    sink.close()


def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im), im.mode


def test_sink_png_writer(tmp_path):
    """Seven frames through TWO slots with the writer thread: submit() waits for the thread instead of raising, and every file decodes
    to the restatement, the 16-bit planes with mode 'I;16'."""
    n, (H, W), (h, w), start = 2, (23, 41), (20, 32), ([2, 3], [4, 9])
    frames = [C.frames(300 + k, n, h, w) for k in range(7)]
    st = start_dev(start)
    names = {p: [[str(tmp_path / ('%s_%d_%d.png' % (p, k, b))) for b in range(n)] for k in range(7)] for p in ('depth', 'validity', 'image')}
    with RawFrameSink(n, h, w, H, W, planes=('image', 'depth', 'validity'), slots=2, writer='png') as sink:
        for k in range(7):
            sink.submit(*[dev(a) for a in frames[k]], start=st, paths={p: names[p][k] for p in names})
            assert sink.in_flight() <= 2
        with pytest.raises(RuntimeError):
            sink.collect()                               # the thread's
    assert sink.in_flight() == 0
    for k in range(7):
        ref = C.restate(*frames[k], (H, W), start)
        for p, key in (('depth', 'depth_u16'), ('validity', 'validity_u16'), ('image', 'image_u8')):
            for b in range(n):
                a, mode = decode(names[p][k][b])
                assert mode == ('RGB' if p == 'image' else 'I;16') and a.dtype == ref[key].dtype and np.array_equal(a, ref[key][b]), (k, p, b)
    # one plane: a plain list of paths; a failure in the thread is raised from the next call
    sink = RawFrameSink(n, h, w, writer='png')
    with pytest.raises(ValueError):
        sink.submit(depth=dev(frames[0][0]))             # no paths
    sink.submit(depth=dev(frames[0][0]), paths=[str(tmp_path / 'no_such_dir' / 'a.png'), str(tmp_path / 'b.png')])
    with pytest.raises(RuntimeError, match='writer thread failed'):
        sink.close()
    assert sink.in_flight() == 0                         # the failed frame's slot was released all the same


def test_golden_fixture_through_the_sink(golden_dir, tmp_path):
    """The inputs the real save_depth / save_validity_map / save_image were given, through the sink: its pinned planes, and the files its
    writer encodes, decode to what the reference's files decode to."""
    g = np.load(os.path.join(golden_dir, 'egress_raw.npz'))
    depth, validity = dev(g['depth'][None, None]), dev(g['validity'][None, None])
    for mult, scale, image, dk, ik in ((256.0, 255.0, dev(g['image'][None]), 'depth_256', 'image'), (1000.0, 1.0, dev(g['image_255'][None]), 'depth_1000', 'image_255')):
        sink = RawFrameSink(1, 9, 13, planes=('depth', 'validity', 'image'), multiplier=mult, image_scale=scale)
        sink.submit(depth, validity, image)
        got = sink.collect()
        for key, ref in (('depth_u16', dk), ('validity_u16', 'validity'), ('image_u8', ik)):
            assert got[key].dtype == g[ref + '_png'].dtype and np.array_equal(got[key][0], g[ref + '_png']), (mult, key)
        sink.release()
        paths = {p: [str(tmp_path / ('%s_%d.png' % (p, int(mult))))] for p in ('depth', 'validity', 'image')}
        with RawFrameSink(1, 9, 13, planes=('depth', 'validity', 'image'), multiplier=mult, image_scale=scale, writer='png') as png:
            png.submit(depth, validity, image, paths=paths)
        for p, ref in (('depth', dk), ('validity', 'validity'), ('image', ik)):
            a, mode = decode(paths[p][0])
            assert mode == str(g[ref + '_mode']) and a.dtype == g[ref + '_png'].dtype and np.array_equal(a, g[ref + '_png']), (mult, p)


def make_model():
    from proxytta.model import ExternalModel_Adapt
    model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
    model._prepare_head(ONE)
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict(ONE).items()})
    opt = torch.optim.Adam(model.adapt_parameters(mode='meta'), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
    model.model.bind_optimizer(opt)
    return model, opt


def test_adapt_submits_behind_its_eval_forward():
    """adapt(..., sink=...) on a 32 x 48 MSG_CHN engine: the same depth and loss_info as without the argument, bit for bit, and the
    collected plane is egress_raw of the returned depth."""
    image, sparse = [torch.from_numpy(x).cuda() for x in synth.synthetic_frame(7, 32, 48, 1)]
    plain, _ = make_model()
    sunk, _ = make_model()
    sink = RawFrameSink(1, 32, 48, 37, 61)
    for _ in range(2):
        d0, i0 = plain.adapt(image, sparse, inner_iter=1)
        d1, i1 = sunk.adapt(image, sparse, inner_iter=1, sink=sink)
        assert torch.equal(d0, d1) and torch.equal(i0, i1)
        got = sink.collect()
        assert got['depth_u16'].shape == (1, 37, 61) and got['depth_u16'][0, :32, :48].any() and not got['depth_u16'][0, 32:].any()
        assert same(egress_raw(depth=d1, dst_size=(37, 61))['depth_u16'], got['depth_u16'])
        sink.release()
    assert sink.in_flight() == 0
