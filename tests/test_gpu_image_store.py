"""GPU: the 8-bit image store — byte expansion (gather), the 8-bit check of the upload, the synthesis read straight out
of the store (adil_synth_store) against the synthesis of the gathered batch, 64-bit row offsets past 4 GB, and the
learners / the evaluation on a byte store against the stream-dtype store of the same 8-bit images."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TABLE = torch.arange(256, dtype=torch.uint8).float().div(255)          # the value of each byte, correctly rounded (CPU)


class _Items(torch.utils.data.Dataset):
    """(image, label) items, `indexed` protocol (imagenet_loading.py:8-18) as the learners use it."""

    def __init__(self, images, labels=None):
        self.images, self.indexed = images, False
        self.labels = torch.zeros(len(images), dtype=torch.int64) if labels is None else labels

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return (i, self.images[i], self.labels[i]) if self.indexed else (self.images[i], self.labels[i])


def _bytes(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _expand(u):
    return TABLE.to(u.device)[u.long()]


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.element_size() == 2 else
                                                                            torch.int32),
                                                                     b.view(torch.int16 if b.element_size() == 2 else
                                                                            torch.int32))


def test_table_is_not_the_reciprocal_product():
    """The store's value table is the correctly rounded quotient, which u * (1/255) is not (126 of 256 differ)."""
    assert int((torch.arange(256).float() * torch.tensor(1 / 255, dtype=torch.float32) != TABLE).sum()) == 126


@pytest.mark.parametrize("p", [192, 150528])
def test_gather_expands_bytes(p):
    from dl_attack_on_imagenet_amd import ops
    r = 600
    store = _bytes((r, p), p).to(DEV)
    store[7, :192] = torch.arange(192, dtype=torch.uint8, device=DEV)     # rows 7 and 8 hold every byte value
    store[8, :64] = torch.arange(192, 256, dtype=torch.uint8, device=DEV)
    f32_store = _expand(store)
    g = torch.Generator().manual_seed(1)
    for b in (1, 33, 512):
        idx = torch.randint(0, r, (b,), generator=g)
        idx[: min(b, 3)] = torch.tensor([5, 7, 8])[: min(b, 3)]
        if b > 4:
            idx[4] = idx[3]                                                 # repeats
        idx = idx.to(DEV)
        out = ops.gather_images(store, idx, dtype=torch.float32)
        assert _bits_equal(out, _expand(store[idx]))
        ob = ops.gather_images(store, idx, dtype=torch.bfloat16)
        assert _bits_equal(ob, ops.gather_images(f32_store, idx, dtype=torch.bfloat16))
    seen = ops.gather_images(store, torch.tensor([7, 8], device=DEV), dtype=torch.float32)
    assert torch.equal(torch.unique(seen).cpu(), TABLE)
    with pytest.raises(ValueError, match="explicit float dtype"):
        ops.gather_images(store, idx)


def test_images_to_u8_and_the_upload_check():
    from dl_attack_on_imagenet_amd import ops
    from dl_attack_on_imagenet_amd.loader import ResidentImages
    u = _bytes((20, 3, 16, 16), 3)
    u.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    x = u.float().div(255)                                              # 8-bit images as ToTensor makes them
    out = torch.empty(u.shape, dtype=torch.uint8, device=DEV)
    assert ops.images_to_u8(x.to(DEV), out) == 0
    assert torch.equal(out.cpu(), u)
    bad = x.clone()
    bad[13, 2, 5, 7] = torch.nextafter(bad[13, 2, 5, 7], torch.tensor(2.0))   # one element, one ulp
    assert ops.images_to_u8(bad.to(DEV), out) == 1
    res = ResidentImages(_Items(x), DEV, torch.uint8, chunk=6)
    assert res.images.dtype == torch.uint8 and res.images.element_size() == 1 and torch.equal(res.images.cpu(), u)
    with pytest.raises(ValueError, match="row 13 "):
        ResidentImages(_Items(bad), DEV, torch.uint8, chunk=6)
    raw = ResidentImages(_Items(u), DEV, torch.uint8, chunk=7)           # bytes (PILToTensor) are taken as they are
    assert torch.equal(raw.images.cpu(), u)
    assert _bits_equal(raw.gather([3, 0, 3]).cpu(), x[[3, 0, 3]])
    assert raw.gather([1], torch.bfloat16).dtype == torch.bfloat16


def _max_err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


@pytest.mark.parametrize("k", [1, 50, 100, 128])
def test_synth_store_matches_the_gathered_synthesis(k):
    from dl_attack_on_imagenet_amd import ops
    g = torch.Generator().manual_seed(k)
    p, b, r = 3136, 33, 80                                              # 24 full 128-pixel tiles + a ragged one
    store = _bytes((r, 1, 56, 56), k).to(DEV)
    idx = torch.randint(0, r, (b,), generator=g).to(DEV)
    d = (-1 + 2 * torch.rand(1, 56, 56, k, generator=g)).to(DEV)
    v = (0.05 * torch.randn(r, k, generator=g)).to(DEV)
    vp = ops.pack_codes(v, idx, b)
    x32 = ops.gather_images(store, idx, dtype=torch.float32)
    xb = ops.gather_images(store, idx, dtype=torch.bfloat16)
    ref0 = (_expand(store[idx].cpu()).double().reshape(b, p) +
            v[idx].double().cpu() @ d.reshape(p, k).double().cpu().t())
    for dc, pc in ((-1.0, False), (8 / 255, False), (-1.0, True), (8 / 255, True)):
        o32 = ops.synth_store(store, idx, d, vp, b, torch.float32, delta_clamp=dc, pixel_clamp=pc)
        assert _bits_equal(o32, ops.synth(x32, d, vp, b, delta_clamp=dc, pixel_clamp=pc)), (dc, pc)
        ob = ops.synth_store(store, idx, d, vp, b, torch.bfloat16, delta_clamp=dc, pixel_clamp=pc)
        old = ops.synth(xb, d, vp, b, delta_clamp=dc, pixel_clamp=pc)
        # one bf16 ulp at the scale of the larger of the pixel and the result: the bf16 path rounds x itself (half an ulp
        # of x), which is a whole ulp of a result one binade below x
        mag = torch.maximum(torch.maximum(old.float().abs(), ob.float().abs()), x32.abs()).clamp_min(2 ** -126)
        ulp = torch.pow(2.0, torch.floor(torch.log2(mag)) - 7)
        assert bool(((ob.float() - old.float()).abs() <= ulp).all()), (dc, pc)
        delta = (ref0 - _expand(store[idx].cpu()).double().reshape(b, p))
        ref = _expand(store[idx].cpu()).double().reshape(b, p) + (delta.clamp(-dc, dc) if dc >= 0 else delta)
        ref = ref.clamp(0, 1) if pc else ref
        assert _max_err(ob.reshape(b, p), ref) <= _max_err(old.reshape(b, p), ref), (dc, pc)
    with pytest.raises(ValueError):
        ops.synth_store(store, idx, d, vp, b + 1, torch.float32)


def test_store_past_4gb():
    """Rows whose byte offset is beyond 2^32: the 64-bit row offsets of adil_synth_store and the gather."""
    from dl_attack_on_imagenet_amd import ops
    r, p, k = 30000, 150528, 50                                           # 4.5 GB of bytes
    store = torch.empty((r, 3, 224, 224), dtype=torch.uint8, device=DEV)
    rows = torch.tensor([r - 1, 29998, 28600, 28531, 0, 28532, r - 1, 29001])
    for i, row in enumerate(rows.tolist()):
        store[row] = _bytes((3, 224, 224), 100 + i).to(DEV)
    assert int(rows.max()) * p > 2 ** 32
    idx = rows.to(DEV)
    g = torch.Generator().manual_seed(9)
    d = (-1 + 2 * torch.rand(3, 224, 224, k, generator=g)).to(DEV)
    vp = ops.pack_codes((0.05 * torch.randn(len(rows), k, generator=g)).to(DEV), None, len(rows))
    x = _expand(store[idx])                                               # the rows copied out with torch
    assert _bits_equal(ops.gather_images(store, idx, dtype=torch.float32), x)
    for dc in (-1.0, 8 / 255):
        assert _bits_equal(ops.synth_store(store, idx, d, vp, len(rows), torch.float32, delta_clamp=dc, pixel_clamp=True),
                           ops.synth(x, d, vp, len(rows), delta_clamp=dc, pixel_clamp=True))
    del store
    torch.cuda.empty_cache()


def _learn(tmp_path, name, images, val, **kw):
    from attacks import ADIL
    from tinynet import make_tinynet
    stores = []

    class Spy(ADIL):
        def _resident(self, dataset, rows=None):
            res = super()._resident(dataset, rows)
            stores.append(res)
            return res
    g = torch.Generator().manual_seed(5)
    n, k = len(images), 6
    d0, v0 = -1 + 2 * torch.rand(3, 32, 32, k, generator=g), torch.rand(n, k, generator=g)
    eb = [[list(range(e, n, 3))[:8], list(range((e + 1) % 3, n, 3))[:8], list(range((e + 2) % 3, n, 3))[:8]]
          for e in range(8)]
    vb = [[[0, 3, 5, 7], [1, 2, 4, 6, 8]] for _ in range(8)]
    Spy(make_tinynet(8).to(DEV), eps=0.3, steps=4, n_atoms=k, batch_size=8, loss="logits", init_d=d0, init_v=v0,
        data_train=_Items(images), data_val=_Items(val), model_name=name, dict_dir=str(tmp_path), epoch_batches=eb,
        val_batches=vb, **kw)
    return torch.load(tmp_path / f"ImageNet_{name}.bin", map_location="cpu"), stores


@pytest.mark.parametrize("method,graph,cache", [("gd", False, True), ("gd", True, True), ("alter", False, False)])
def test_learning_on_a_byte_store_is_bitwise_the_float_store(tmp_path, method, graph, cache):
    images = _bytes((24, 3, 32, 32), 11).float().div(255)
    val = _bytes((9, 3, 32, 32), 12).float().div(255)
    kw = dict(method=method, use_graph=graph, cache_labels=cache, steps_in=1)
    a, sa = _learn(tmp_path, "f32", images, val, **kw)
    b, sb = _learn(tmp_path, "u8", images, val, image_store="uint8", **kw)
    assert all(s.images.dtype == torch.float32 for s in sa)
    assert len(sb) == 2 and all(s.images.dtype == torch.uint8 and s.images.element_size() == 1 for s in sb)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3] and float(a[4]) == float(b[4])


def test_learner_refuses_fp8_with_a_byte_store():
    from dl_attack_on_imagenet_amd import engine
    from dl_attack_on_imagenet_amd.loader import ResidentImages
    from tinynet import make_tinynet
    res = ResidentImages(_Items(_bytes((8, 3, 32, 32), 2)), DEV, torch.uint8)
    learner = engine.DictionaryLearner(torch.zeros(3, 32, 32, 4, device=DEV), torch.zeros(8, 4, device=DEV), 0.1,
                                       fp8_synth=True)
    with pytest.raises(ValueError, match="fp8"):
        learner.step(make_tinynet(1).to(DEV), res, torch.arange(4, device=DEV))


def test_performance_over_a_byte_store():
    import performance as perf
    from dl_attack_on_imagenet_amd.loader import ResidentBatches
    from tinynet import make_tinynet
    net = make_tinynet(6).to(DEV)
    u = _bytes((22, 3, 32, 32), 13)
    x = u.float().div(255)
    labels = net(x.to(DEV)).argmax(-1).cpu()
    labels[::4] = (labels[::4] + 1) % 10                                  # some misclassified rows are filtered out

    class FixedAttack:
        device = torch.device(DEV)

        def __call__(self, x, y):
            return (x + 0.08 * torch.sign(x - 0.5)).clamp(0, 1)
    ref = perf.performance(FixedAttack(), net, ResidentBatches(_Items(x), labels, 5, DEV))
    for items in (x, u):
        out = perf.performance(FixedAttack(), net, ResidentBatches(_Items(items), labels, 5, DEV, dtype=torch.uint8))
        assert float(out["fooling_rate"]) == float(ref["fooling_rate"])
        assert float(out["rmse"]) == float(ref["rmse"]) and float(out["mse"]) == float(ref["mse"])
