"""CPU-only checks of the cellularity scoring feature: the view ids, the argument checks of the three C entries, the fixture's
self-consistency and the host side of the drivers (utils.eval.predict_breastpathq / cls_scores, utils.dataset.Dataset)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import views_oracle as VO
from wsi_segmentation_pipeline_amd import engine as E
from wsi_segmentation_pipeline_amd import native


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def test_reference_views_are_ids_0_1_2_5():
    assert E.VIEWS_REFERENCE == VO.VIEWS_REFERENCE == (0, 1, 2, 5) and (E.VIEW_T, E.VIEW_FY, E.VIEW_FX) == (1, 2, 4)
    image = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).view(2, 3, 5, 7)
    augmented_set = [image, image.transpose(2, 3), image.flip(2), image.transpose(2, 3).flip(3)]
    for v, ref in zip(E.VIEWS_REFERENCE, augmented_set):
        assert np.array_equal(VO.apply_view(image.numpy(), v, (2, 3)), ref.numpy()), v
    from utils.eval import torch_view
    for v in range(8):
        assert np.array_equal(torch_view(image, v).numpy(), VO.apply_view(image.numpy(), v, (2, 3))), v
    s = np.arange(5 * 7).reshape(5, 7)                                   # the index formula of include/wsi_hip.h
    for v in range(8):
        hv, wv = VO.view_shape(v, 5, 7)
        got = VO.apply_view(s, v)
        assert got.shape == (hv, wv)
        for y in range(hv):
            for x in range(wv):
                y2, x2 = (hv - 1 - y if v & 2 else y), (wv - 1 - x if v & 4 else x)
                sy, sx = (x2, y2) if v & 1 else (y2, x2)
                assert got[y, x] == s[sy, sx], (v, y, x)
    assert np.array_equal(VO.apply_view(s, 5), np.array([[s[5 - 1 - x, y] for x in range(5)] for y in range(7)]))


def test_view_ids_form_a_group():
    idx = np.arange(16).reshape(4, 4)
    images = [VO.apply_view(idx, v).tobytes() for v in range(8)]
    assert len(set(images)) == 8
    table = [[VO.compose(a, b) for b in range(8)] for a in range(8)]     # closed: compose() finds an id for every pair
    assert all(sorted(row) == list(range(8)) for row in table)           # every row a permutation: inverses exist
    assert all(table[0][v] == v == table[v][0] for v in range(8))        # 0 is the identity
    for a, b, c in ((1, 2, 5), (5, 3, 6), (7, 1, 4)):
        assert VO.compose(VO.compose(a, b), c) == VO.compose(a, VO.compose(b, c))


def test_view_list_rules():
    assert E.view_ids((0, 0, 7)) == [0, 0, 7]
    for bad in ((), (0,) * 9, (8,), (-1,)):
        with pytest.raises(ValueError):
            E.view_ids(bad)
    assert E.view_groups([0, 1, 2, 5], 64, 64) == [[0, 1, 2, 3]]
    assert E.view_groups([0, 1, 2, 5], 64, 96) == [[0, 2], [1, 3]]
    assert E.view_groups([1, 5], 64, 96) == [[0, 1]]


def test_views_bad_arguments_return_einval(lib):
    """Every -22 case of wsi_tile_views_u8 / wsi_views_f32, without a device: the pointers are never followed."""
    P = C.c_void_p(4096)
    ids = lambda *v: (C.c_int * len(v))(*v)
    ok = dict(slide=P, pitch=3 * 200 + 8, sh=140, sw=200, xy=P, n=2, ph=32, pw=64, views=ids(0, 2), nv=2, out=P)

    def u8(**kw):
        a = dict(ok, **kw)
        return lib.wsi_tile_views_u8(a['slide'], a['pitch'], a['sh'], a['sw'], a['xy'], a['n'], a['ph'], a['pw'], a['views'], a['nv'], a['out'], None)
    for kw in (dict(slide=None), dict(xy=None), dict(views=None), dict(out=None), dict(n=0), dict(n=-1), dict(ph=0), dict(pw=-32), dict(ph=48),
               dict(pw=33), dict(nv=0), dict(nv=9, views=ids(*[0] * 9)), dict(views=ids(0, 8)), dict(views=ids(-1, 0)), dict(pitch=3 * 200 - 1),
               dict(views=ids(0, 1)), dict(views=ids(2, 5))):
        assert u8(**kw) == -22, kw

    def f32(inp=P, n=2, h=32, w=64, views=ids(0, 2), nv=2, out=P):
        return lib.wsi_views_f32(inp, n, h, w, views, nv, out, None)
    for kw in (dict(inp=None), dict(out=None), dict(views=None), dict(n=0), dict(h=0), dict(w=40), dict(h=-32), dict(nv=0), dict(nv=9),
               dict(views=ids(0, 9)), dict(views=ids(1, 2)), dict(views=ids(4, 7))):
        assert f32(**kw) == -22, kw


def test_mlp_views_bad_arguments_return_einval(lib):
    P = C.c_void_p(4096)
    ok = dict(feat=P, n=3, nv=4, f=64, w1=P, b1=P, j=16, w2=P, b2=P, k=1, mean=P)

    def mlp(**kw):
        a = dict(ok, **kw)
        return lib.wsi_mlp_views(a['feat'], a['n'], a['nv'], a['f'], a['w1'], a['b1'], a['j'], a['w2'], a['b2'], a['k'], 0, 0.0, 1.0, None, a['mean'], None)
    for kw in (dict(feat=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(mean=None), dict(n=0), dict(f=0), dict(k=0),
               dict(j=-1), dict(nv=0), dict(nv=9), dict(j=0, w2=None), dict(j=0, b2=None)):
        assert mlp(**kw) == -22, kw


def test_fixture_is_self_consistent():
    """tests/golden/cellularity_views.npz against the CPU restatement (1e-5), the stated accumulation order, the clamp and the
    properties the generator asserted."""
    z = VO.load_fixture()
    assert tuple(z['views']) == VO.VIEWS_REFERENCE
    clamped = []
    for name in ('sq', 'ns'):
        pv, logits = VO.restate(z['sd'], z['reg'], z['cls'], z['u8_' + name])
        assert np.abs(pv - z['reg_views_' + name]).max() <= 1e-5 and np.abs(logits - z['cls_views_' + name]).max() <= 1e-5
        assert np.array_equal(VO.mean_views(z['reg_views_' + name]), z['reg_mean_' + name])
        assert np.array_equal(np.minimum(np.maximum(z['reg_mean_' + name], 0.0), 1.0), z['reg_clamped_' + name])
        assert max(np.abs(z['reg_views_' + name]).max(), np.abs(z['cls_views_' + name]).max()) <= 16.0
        for a in range(4):
            for b in range(a + 1, 4):
                assert np.abs(z['reg_views_' + name][:, a] - z['reg_views_' + name][:, b]).max() >= 0.02, (name, a, b)
        clamped.append(z['reg_clamped_' + name])
    c = np.concatenate(clamped)
    assert (c == 0.0).any() and ((c > 0.0) & (c < 1.0)).any()


def test_cls_scores_hand_counted():
    from utils.eval import cls_scores
    # TP 2 (items 0, 3), FP 1 (item 1), FN 1 (item 2), TN 1; a class-2 item counts as "not 1" on either side
    acc, f1 = cls_scores([1, 0, 1, 1, 0, 2], [1, 1, 0, 1, 0, 2])
    assert acc == pytest.approx(4 / 6) and f1 == pytest.approx(2 * 2 / (2 * 2 + 1 + 1))
    assert cls_scores([0, 0], [0, 0]) == (1.0, 0.0)                      # no positive anywhere: F1 defined as 0
    assert cls_scores([1, 1], [1, 1]) == (1.0, 1.0)
    assert cls_scores([1, 1, 0], [0, 0, 0]) == (pytest.approx(1 / 3), 0.0)
    assert cls_scores([2, 1], [1, 2])[1] == 0.0                          # TP 0, FP 1, FN 1
    with pytest.raises(ValueError):
        cls_scores([1, 0], [1])


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_patch_dataset_and_iterator(tmp_path, monkeypatch):
    from myargs import args
    from utils import dataset as D
    from utils.preprocessing import standard_augmentor
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (40, 48, 3), dtype=np.uint8) for _ in range(3)]
    for i, a in enumerate(imgs):
        _png(str(tmp_path / ('im%d.png' % i)), a)
    lab = rng.integers(0, 4, (40, 48), dtype=np.uint8)
    _png(str(tmp_path / 'lab2.png'), lab)
    gt = {'caseA': {0: {'wsi': str(tmp_path / 'im0.png'), 'label': 1}, 1: {'wsi': str(tmp_path / 'im1.png'), 'label': 0.25}},
          'caseB': {7: {'wsi': str(tmp_path / 'im2.png'), 'label': str(tmp_path / 'lab2.png')}}}
    np.save(str(tmp_path / 'gt.npy'), gt, allow_pickle=True)
    ds = D.Dataset(str(tmp_path), eval=True, duplicate_dataset=3)
    assert len(ds) == 3
    aug = standard_augmentor(True)
    for i, (flags, code) in enumerate((((True, False, False), 1), ((False, True, False), 0.25), ((False, False, True), -1))):
        image, label, is_cls, is_reg, is_seg, cls_code = ds[i]
        assert torch.equal(image, aug(imgs[i])) and image.dtype == torch.float32 and tuple(image.shape) == (3, 40, 48)
        assert (is_cls, is_reg, is_seg) == flags and cls_code == code
        assert label.dtype == torch.int64 and np.array_equal(label.numpy(), lab if i == 2 else np.zeros((40, 48)))
    monkeypatch.setattr(args, 'tile_w', 32)
    monkeypatch.setattr(args, 'tile_h', 24)
    train = D.Dataset(str(tmp_path), eval=False, duplicate_dataset=2)
    assert len(train) == 6 and [d['wsi'] for d in train.datalist[:2]] == [str(tmp_path / 'im0.png')] * 2
    image, label, *_ = train[4]
    assert tuple(image.shape) == (3, 24, 32) and tuple(label.shape) == (24, 32)
    monkeypatch.setattr(args, 'workers', 0)
    monkeypatch.setattr(args, 'batch_size', 2)
    monkeypatch.setattr(torch.utils.data.DataLoader, '__init__', _no_pin(torch.utils.data.DataLoader.__init__))
    gt2 = {'caseA': {i: {'wsi': str(tmp_path / ('im%d.png' % i)), 'label': i % 2} for i in range(3)}}
    np.save(str(tmp_path / 'gt.npy'), gt2, allow_pickle=True)
    it = D.GenerateIterator(str(tmp_path), eval=True)
    batches = list(it)
    assert [int(b[0].shape[0]) for b in batches] == [2, 1]
    codes = sorted(int(c) for b in batches for c in b[5])
    assert codes == [0, 0, 1] and all(bool(v) for b in batches for v in b[2])


def _no_pin(init):
    """DataLoader.__init__ with pin_memory off: this test has no device to pin for"""
    def wrapped(self, *a, **kw):
        kw['pin_memory'] = False
        return init(self, *a, **kw)
    return wrapped


def test_breastpathq_host_part(tmp_path, monkeypatch):
    """Row order, resize and CSV text of predict_breastpathq with an injected scoring function."""
    from PIL import Image
    from myargs import args
    from utils import eval as U
    monkeypatch.setattr(args, 'tile_w', 64)
    monkeypatch.setattr(args, 'tile_h', 32)
    rng = np.random.default_rng(9)
    order = [(7, 2), (3, 1), (7, 1), (12, 5), (3, 9)]
    arrays = {}
    for k, (a, b) in enumerate(order):
        shape = (32, 64, 3) if k != 3 else (48, 80, 3)                    # one region really gets resized
        arrays[(a, b)] = rng.integers(0, 256, shape, dtype=np.uint8)
        Image.fromarray(arrays[(a, b)]).save(str(tmp_path / ('%d_%d.tif' % (a, b))))
    labels = tmp_path / 'labels.csv'
    labels.write_text('slide,rid,y\n' + ''.join('%d,%d,0.5\n' % ab for ab in order))
    assert U.breastpathq_rows(str(labels)) == order
    seen = []

    def score(u8):
        seen.append(u8.copy())
        return u8.reshape(u8.shape[0], -1).mean(1) / 255.0

    out = tmp_path / 'out.csv'
    rows = U.predict_breastpathq(None, 3, str(tmp_path), str(labels), out_csv=str(out), batch=2, score=score)
    assert [int(s.shape[0]) for s in seen] == [2, 2, 1] and all(s.shape[1:] == (32, 64, 3) and s.dtype == np.uint8 for s in seen)
    got = np.concatenate(seen)
    for k, ab in enumerate(order):
        want = arrays[ab] if k != 3 else np.asarray(Image.fromarray(arrays[ab]).resize((64, 32), Image.BILINEAR))
        assert np.array_equal(got[k], want), ab
    assert [(a, b) for a, b, _ in rows] == order
    want_p = [np.float32(got[k].mean() / 255.0) for k in range(5)]
    assert [p for _, _, p in rows] == want_p
    assert out.read_bytes().decode() == 'slide,rid,p\r\n' + ''.join('%d,%d,%s\r\n' % (a, b, p) for (a, b), p in zip(order, want_p))
    monkeypatch.chdir(tmp_path)
    U.predict_breastpathq(None, 11, str(tmp_path), str(labels), batch=8, score=score)
    assert (tmp_path / 'Ozan_Results_11.csv').read_bytes() == out.read_bytes()
