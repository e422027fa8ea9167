"""ptta_ingest_raw (proxytta.ingest.ingest_raw) and RawFrameStager on the GPU: every comparison is torch.equal against the numpy
restatement of the reference's loader (tests/ingest_cases.py, itself held bit for bit to the real functions' outputs by
tests/test_ingest_cpu.py).  Every output is a view inside a larger buffer filled with a sentinel no result can equal; the sentinel is
checked on both sides of the view after every call."""
import os
import zlib

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.ingest import PLANES, ingest_raw
from proxytta.staging import RawFrameStager
from tests import ingest_cases as C
from tests.util import make_engine

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0          # every result is >= 0
PAD = 64                     # floats on each side of a view: 256 bytes, so a view keeps the buffer's 16-byte alignment
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1,
          max_input_depth=80.0)


def dev16(a):
    """uint16 numpy -> device tensor carrying the same bits (int16: the library reads the plane as unsigned)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


class Guarded:
    """fp32 output planes as views inside sentinel-filled buffers"""

    def __init__(self, n, h, w, planes, pad=PAD):
        self.buf, self.out, self.pad = {}, {}, pad
        for k in planes:
            shape = (n, 3 if k == 'image' else 1, h, w)
            numel = int(np.prod(shape))
            self.buf[k] = torch.full((pad + numel + PAD,), SENTINEL, dtype=torch.float32, device='cuda')
            self.out[k] = self.buf[k][pad:pad + numel].view(shape)

    def margins_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:self.pad] == SENTINEL).all()) and bool((b[self.pad + self.out[k].numel():] == SENTINEL).all()) for k, b in self.buf.items())

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((b == SENTINEL).all()) for b in self.buf.values())


def expected(image, sparse, gt, size, start, multiplier=256.0):
    ref = {}
    if image is not None:
        ref['image'] = C.restate_image(image, size, start)
    if sparse is not None:
        ref['sparse'], ref['validity'] = C.restate_depth(sparse, size, start, multiplier)
    if gt is not None:
        ref['gt'], ref['gt_validity'] = C.restate_depth(gt, size, start, multiplier)
    return ref


def check(image, sparse, gt, size, start, multiplier=256.0, planes=None, pad=PAD, to_dev=None):
    """One call on guarded outputs; every plane asked for equals the restatement and the sentinels stand."""
    given = [a for a in (image, sparse, gt) if a is not None]
    n, H, W = given[0].shape[:3]
    h, w = (H, W) if size is None else size
    ref = expected(image, sparse, gt, size, start, multiplier)
    planes = [k for k in PLANES if k in ref] if planes is None else planes
    g = Guarded(n, h, w, planes, pad)
    assert g.margins_intact()
    to_dev = to_dev or {}
    dev = [None if a is None else to_dev.get(k, dev16 if a.dtype == np.uint16 else (lambda x: torch.from_numpy(x).cuda()))(a)
           for k, a in zip(('image', 'sparse', 'gt'), (image, sparse, gt))]
    st = None if start is None else tuple(torch.tensor(s, dtype=torch.int32).cuda() for s in start)
    got = ingest_raw(*dev, size=size, start=st, multiplier=multiplier, out=g.out)
    assert g.margins_intact()
    assert sorted(got) == sorted(planes)
    for k in planes:
        assert got[k].data_ptr() == g.out[k].data_ptr()
        assert torch.equal(got[k].cpu(), torch.from_numpy(ref[k])), k
    return got


@pytest.mark.parametrize('case', C.CASES, ids=[c[0] for c in C.CASES])
def test_case_table(case):
    name, n, (H, W), size, start, _ = case
    image, sparse, gt = C.raw_frames(zlib.crc32(name.encode()), n, H, W)
    check(image, sparse, gt, size, start)


def test_out_of_range_starts_clamp_as_crop_flip_does():
    """The window of the ingest = ptta_crop_flip's crop of the whole ingested frame, for starts below zero, inside and beyond the sample."""
    name, n, (H, W), (h, w), start, _ = [c for c in C.CASES if c[0] == 'starts_out_of_range'][0]
    image, sparse, _ = C.raw_frames(80, n, H, W)
    im, sp = torch.from_numpy(image).cuda(), dev16(sparse)
    sy, sx = (torch.tensor(s, dtype=torch.int32).cuda() for s in start)
    whole = ingest_raw(im, sp)
    got = ingest_raw(im, sp, size=(h, w), start=(sy, sx))
    lib = _lib.load()
    for k in ('image', 'sparse', 'validity'):
        c = whole[k].shape[1]
        crop = torch.full((n, c, h, w), SENTINEL, dtype=torch.float32, device='cuda')
        rc = lib.ptta_crop_flip(_lib.ptr(whole[k]), _lib.ptr(crop), n, c, H, W, h, w, _lib.ptr(sy), _lib.ptr(sx), None, None,
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and torch.equal(got[k], crop), k


@pytest.mark.parametrize('multiplier', [256.0, 1000.0])
def test_division_over_all_65536_values(multiplier):
    """Every 16-bit value through the 16-byte path (256 x 256) and the one-pixel path (a 254 x 259 plane holding them all)."""
    every = np.arange(65536, dtype=np.uint16)
    check(None, every.reshape(1, 256, 256), None, None, None, multiplier)
    plane = np.zeros(254 * 259, dtype=np.uint16)
    plane[:65536] = every[::-1]
    check(None, plane.reshape(1, 254, 259), None, None, None, multiplier)


def test_extreme_image_values_and_null_combinations():
    image, sparse, gt = C.raw_frames(77, 2, 6, 12)
    image[0, ::2, ::2], image[0, 1::2, 1::2], image[1, 0], image[1, -1] = 0, 255, 255, 0
    assert set(check(image, None, None, None, None)) == {'image'}                                     # image only
    assert set(check(None, sparse, None, None, None, planes=['sparse'])) == {'sparse'}                # sparse without validity
    assert set(check(None, None, gt, (5, 8), ([1, 0], [3, 4]))) == {'gt', 'gt_validity'}              # ground truth only
    assert set(check(None, None, gt, None, None, planes=['gt'])) == {'gt'}
    assert set(check(image, sparse, gt, None, None, planes=['image', 'sparse', 'gt', 'gt_validity'])) == {'image', 'sparse', 'gt', 'gt_validity'}
    # without `out` the wrapper allocates every plane of the inputs given
    got = ingest_raw(torch.from_numpy(image).cuda(), dev16(sparse))
    assert sorted(got) == ['image', 'sparse', 'validity'] and torch.equal(got['image'].cpu(), torch.from_numpy(C.restate_image(image)))


def test_unaligned_bases():
    """Inputs whose first byte sits at every offset of a word (views into larger buffers), so rows begin at every misalignment and the
    first row lies at the unaligned front of its array; outputs off the 16-byte grid take the one-pixel path with the same results."""
    image, sparse, gt = C.raw_frames(78, 2, 7, 16)
    for off in range(4):
        def shifted_u8(a, off=off):
            big = torch.zeros(a.size + 8, dtype=torch.uint8, device='cuda')
            big[off:off + a.size] = torch.from_numpy(a).cuda().flatten()
            return big[off:off + a.size].view(a.shape)

        def shifted_u16(a, off=off):
            big = torch.zeros(a.size + 4, dtype=torch.int16, device='cuda')
            big[off % 2:off % 2 + a.size] = dev16(a).flatten()
            return big[off % 2:off % 2 + a.size].view(a.shape)
        for size, start in ((None, None), ((5, 12), ([0, 2], [1, 4])), ((7, 8), ([0, 0], [8, 5]))):
            check(image, sparse, gt, size, start, to_dev={'image': shifted_u8, 'sparse': shifted_u16, 'gt': shifted_u16})
    check(image, sparse, gt, (5, 12), ([2, 1], [3, 0]), pad=PAD + 1)


def test_golden_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ingest_raw.npz'))
    got = ingest_raw(torch.from_numpy(g['image_u8'][None]).cuda(), dev16(g['depth_u16'][None]), dev16(g['depth_u16'][None]))
    for k, key in (('image', 'image'), ('sparse', 'depth_256'), ('validity', 'validity'), ('gt', 'depth_v'), ('gt_validity', 'validity')):
        assert torch.equal(got[k][0].cpu(), torch.from_numpy(g[key])), k
    got = ingest_raw(sparse_u16=dev16(g['depth_u16'][None]), multiplier=1000.0)
    assert torch.equal(got['sparse'][0].cpu(), torch.from_numpy(g['depth_1000']))


@pytest.mark.parametrize('case', C.FULL, ids=[c[0] for c in C.FULL])
def test_full_size(case):
    name, n, (H, W), size, start = case
    image, sparse, gt = C.raw_frames(zlib.crc32(name.encode()), n, H, W, density=0.05)
    check(image, sparse, gt, size, start)


def test_refusals_leave_the_outputs_untouched():
    n, H, W, h, w = 2, 6, 8, 4, 8
    image, sparse, gt = C.raw_frames(79, n, H, W)
    im, sp, gd = torch.from_numpy(image).cuda(), dev16(sparse), dev16(gt)
    g = Guarded(n, h, w, PLANES)
    o = g.out
    refused = pytest.raises(RuntimeError, match=r'\(-22\)')
    # through the wrapper
    with refused:
        ingest_raw(None, sp, None, size=(h, w), out={'image': o['image'], 'sparse': o['sparse']})          # an output without its input
    with refused:
        ingest_raw(None, sp, None, size=(h, w), out={'sparse': o['sparse'], 'gt_validity': o['gt_validity']})
    with refused:
        ingest_raw(im, None, None, size=(h, w), out={'image': o['image'], 'validity': o['validity']})
    with refused:
        ingest_raw(im, sp, None, size=(h, w), out={'image': o['image']})                                   # an input with no output
    with refused:
        ingest_raw(im, sp, None, size=(h, w), out={'image': o['image'], 'validity': o['validity']})        # (validity alone is not sparse's output)
    with refused:
        ingest_raw(None, None, None, size=(h, w), out={'image': o['image']})                               # no input at all
    with refused:
        ingest_raw()
    with refused:
        ingest_raw(im, sp, gd, size=(0, w))
    with refused:
        ingest_raw(im, sp, gd, size=(H + 1, W))
    for bad in (0.0, -256.0, float('inf'), float('nan')):
        with refused:
            ingest_raw(im, sp, gd, size=(h, w), multiplier=bad, out=o)
    # every check of the entry point on its own, with all five outputs bound
    lib = _lib.load()
    ok = dict(n=n, H=H, W=W, h=h, w=w, multiplier=256.0)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.ptta_ingest_raw(_lib.ptr(im), _lib.ptr(sp), _lib.ptr(gd), *[_lib.ptr(o[k]) for k in PLANES], a['n'], a['H'], a['W'], a['h'], a['w'],
                                 None, None, a['multiplier'], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('ptta_ingest_raw failed (%d)' % rc)
    for kw in (dict(n=0), dict(n=-1), dict(H=0, h=0), dict(W=0, w=0), dict(h=0), dict(w=0), dict(h=-4), dict(h=H + 1), dict(w=W + 1),
               dict(multiplier=0.0), dict(multiplier=-1.0), dict(multiplier=float('inf')), dict(multiplier=float('nan'))):
        with refused:
            call(**kw)
    assert g.untouched()
    call()                                                                                                  # the same call, valid: it runs
    assert g.margins_intact() and torch.equal(o['image'].cpu(), torch.from_numpy(C.restate_image(image, (h, w))))


# ---- host staging of raw frames ----------------------------------------------------------------------------
def test_raw_stager_delivers_frames_in_order_and_reuses_slots():
    n, H, W, h, w = 2, 43, 69, 40, 64
    frames = [C.raw_frames(100 + k, n, H, W) for k in range(7)]
    starts = [([k % 4, 3 - k % 4], [k, 5 - k % 5]) for k in range(7)]
    st = RawFrameStager(n, H, W, h, w, ground_truth=True)
    assert st.bytes_per_frame == st.layout['bytes'] and st.slots == 3
    slots_seen = []
    st.submit(*frames[0], start=starts[0])
    for k in range(7):
        if k + 1 < 7:
            st.submit(*frames[k + 1], start=starts[k + 1])         # frame k+1 travels while frame k is consumed
        got = st.acquire()
        slots_seen.append(got[0].data_ptr())
        kept = [t.clone() for t in got]
        st.release()
        ref = expected(*frames[k], (h, w), starts[k])
        assert len(kept) == 5 and all(t.dtype == torch.float32 for t in kept)
        for t, key in zip(kept, PLANES):
            assert torch.equal(t.cpu(), torch.from_numpy(ref[key])), (k, key)
    assert slots_seen[:3] == slots_seen[3:6] and slots_seen[6] == slots_seen[0] and len(set(slots_seen)) == 3
    assert st.in_flight() == 0
    with pytest.raises(RuntimeError):
        st.acquire()
    for k in range(3):
        st.submit(*frames[k])
    with pytest.raises(RuntimeError):
        st.submit(*frames[3])                                      # all slots in flight
    with pytest.raises(ValueError):
        RawFrameStager(n, H, W, h, w).submit(*frames[0])           # ground truth handed to a stager built without it
    # without ground truth and without a window: (image, sparse) of the whole source, a wider integer array narrowed on the way
    plain = RawFrameStager(n, H, W)
    plain.submit(frames[1][0], frames[1][1].astype(np.int32))
    im, sd = plain.acquire()
    assert torch.equal(im.cpu(), torch.from_numpy(C.restate_image(frames[1][0]))) and torch.equal(sd.cpu(), torch.from_numpy(C.restate_depth(frames[1][1])[0]))
    plain.release()


def test_raw_staged_sequence_equals_resident_sequence():
    """Five MSG_CHN steps fed through RawFrameStager, plain and with the next slot announced on the engine's prefix stream, leave
    exactly the loss infos and adapted parameters of five steps on the restated fp32 frames resident in HBM."""
    n, H, W, h, w = 1, 70, 101, 64, 96
    rng = np.random.default_rng(9)
    raws = [(rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8),
             (rng.integers(256, 20000, size=(n, H, W)) * (rng.random((n, H, W)) < 0.05)).astype(np.uint16)) for _ in range(5)]
    starts = [([k], [2 * k + 1]) for k in range(5)]

    def run(staged):
        eng, _, adapted = make_engine(n, h, w, 'fp32', HP)
        infos = []
        if staged:
            st = RawFrameStager(n, H, W, h, w)
            st.submit(*raws[0], start=starts[0])
            for k in range(5):
                if k + 1 < 5:
                    st.submit(*raws[k + 1], start=starts[k + 1])
                im, sd = st.acquire()
                nxt = st.peek_next(eng.prefix_stream()) if staged == 'pipelined' else None
                infos.append(eng.step(im, sd, next_frame=nxt)[0])
                st.release()
        else:
            for k in range(5):
                im = torch.from_numpy(C.restate_image(raws[k][0], (h, w), starts[k])).cuda()
                sd = torch.from_numpy(C.restate_depth(raws[k][1], (h, w), starts[k])[0]).cuda()
                infos.append(eng.step(im, sd)[0])
        torch.cuda.synchronize()
        res = torch.stack(infos).cpu(), {k: v[0].detach().cpu().clone() for k, v in adapted.items()}
        eng.close()
        return res
    ia, pa = run(False)
    assert bool(torch.isfinite(ia).all())
    for mode in (True, 'pipelined'):
        ib, pb = run(mode)
        assert torch.equal(ia, ib), mode
        for k in pa:
            assert torch.equal(pa[k], pb[k]), (mode, k)
