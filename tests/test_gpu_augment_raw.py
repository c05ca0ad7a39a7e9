"""GPU: training crops from stored uint8 images (`ebc_augment_crops_raw`, `CropAugment` with raw sources,
`RawCropLoader`).  The yardstick of every pixel comparison is the existing float path on `u8.float() / 255` of the same
image, compared with `torch.equal`: the raw horizontal pass converts a byte as `(float)u / 255.0f` and runs the float
pass's fmaf chain over the float pass's taps, and every later launch is the float path's own.  The oracle bars are
those of tests/test_gpu_augment.py (2e-5 unnormalised resize, 1e-4 after the whole pipeline)."""
import pytest
import torch

from conftest import ANCHORS_NWPU, BINS, golden

pytestmark = pytest.mark.gpu

HWC, CHW = 0, 1


def _u8(h, w, seed):
    """A [3, H, W] uint8 image; `_as(x, layout)` gives the stored form."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g)


def _as(chw, layout):
    return chw.permute(1, 2, 0).contiguous() if layout == HWC else chw.clone()


def _f32(chw):
    return (chw.float() / 255).cuda()


def _fresh_device(t):
    """`t` in a device allocation of exactly its own bytes."""
    buf = torch.empty(t.numel(), dtype=torch.uint8, device="cuda")
    buf.copy_(t.reshape(-1))
    return buf.view(t.shape)


def _sweep_plans():
    from ebc_amd.transforms import CropPlan
    plans = []
    for top in (0, 5):
        for left in range(8):
            for cw in range(13, 21):
                plans.append(CropPlan(0, top, left, 16, cw, None, len(plans) % 2 == 1))
    plans.append(CropPlan(0, 7, 17, 16, 20, None, False))          # ends on the image's last byte
    plans.append(CropPlan(0, 7, 24, 16, 13, None, True))
    return plans


@pytest.fixture(scope="module")
def sweep():
    from ebc_amd.transforms import CropAugment
    aug = CropAugment(16, jitter_prob=0.0, blur_prob=0.0, noise_prob=0.0)
    img = _u8(23, 37, 3)
    plans = _sweep_plans()
    want = aug.apply([_f32(img)], plans, normalize=False).cpu()
    return aug, img, plans, want


@pytest.mark.parametrize("where", ["device", "cpu"])
@pytest.mark.parametrize("layout", [HWC, CHW])
def test_alignment_sweep(sweep, layout, where):
    """Every (first byte mod 4, span bytes mod 4) of a staged row, in place on the device (the image a fresh
    allocation of exactly H*W*3 bytes, one window ending on its last byte) and packed from the CPU."""
    aug, img, plans, want = sweep
    H, W = 23, 37
    pairs = set()
    for p in plans:
        start = (p.top * W + p.left) * 3 if layout == HWC else p.top * W + p.left
        pairs.add((start % 4, (p.crop_w * (3 if layout == HWC else 1)) % 4))
    assert len(pairs) == 16
    assert any(p.top + p.crop_h == H and p.left + p.crop_w == W for p in plans)
    raw = _as(img, layout)
    src = _fresh_device(raw) if where == "device" else raw
    assert src.numel() == H * W * 3
    got = aug.apply([src], plans, normalize=False).cpu()
    assert torch.equal(got, want)


@pytest.mark.parametrize("layout", [HWC, CHW])
def test_neighbours_do_not_leak_in(sweep, layout):
    """The image inside a larger device buffer, at an odd byte: what surrounds it does not reach the result."""
    aug, img, plans, want = sweep
    raw = _as(img, layout)
    outs = []
    for fill in (0, 255):
        buf = torch.full((raw.numel() + 64,), fill, dtype=torch.uint8, device="cuda")
        view = buf[13:13 + raw.numel()].view(raw.shape)
        view.copy_(raw)
        outs.append(aug.apply([view], plans, normalize=False).cpu())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], want)


REAL = [(300, 401), (512, 700), (230, 261), (150, 180)]


def _real_plans(aug, seed=5, n_per=3):
    torch.manual_seed(seed)
    plans = []
    for i, (h, w) in enumerate(REAL):
        for _ in range(n_per):
            p, _ = aug.plan_crop(i, h, w, torch.rand(20, 2) * torch.tensor([w, h], dtype=torch.float32))
            plans.append(p)
    return plans


@pytest.mark.parametrize("arrangement", [0, 1])
def test_real_sizes_and_mixed_batch(arrangement):
    """One `apply` call over uint8 HWC on the device, uint8 CHW on the CPU and a float32 device image; the 150 x 180
    image takes the pre-resize branch (packed whole from the CPU in one arrangement, read in place in the other)."""
    from ebc_amd.transforms import CropAugment
    from oracle import augment_ref as ref
    imgs = [_u8(h, w, 10 + i) for i, (h, w) in enumerate(REAL)]
    floats = [_f32(x) for x in imgs]
    kinds = [("hwc", "cuda"), ("chw", "cpu"), ("f32", "cuda"), ("hwc", "cpu")] if arrangement == 0 else \
            [("chw", "cpu"), ("f32", "cuda"), ("hwc", "cpu"), ("chw", "cuda")]
    mixed = []
    for x, f, (kind, where) in zip(imgs, floats, kinds):
        mixed.append(f if kind == "f32" else _as(x, HWC if kind == "hwc" else CHW).to(where))
    plain = CropAugment(224, 1.0, 2.0, jitter_prob=0.0, blur_prob=0.0, noise_prob=0.0)
    plans = _real_plans(plain)
    assert all(p.pre_resize is not None for p in plans[9:]) and any(p.pre_resize is None for p in plans[:9])
    got = plain.apply(mixed, plans, normalize=False).cpu()
    assert torch.equal(got, plain.apply(floats, plans, normalize=False).cpu())
    cpu_floats = [x.float() / 255 for x in imgs]
    assert (got - ref.apply_plans(cpu_floats, plans, (224, 224), normalize=False)).abs().max().item() < 2e-5
    full = CropAugment(224, 1.0, 2.0, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, saltiness=0.02,
                       spiciness=0.02, jitter_prob=1.0, blur_prob=1.0, noise_prob=1.0)
    plans = _real_plans(full, seed=6)
    got = full.apply(mixed, plans).cpu()
    assert torch.equal(got, full.apply(floats, plans).cpu())
    exp = ref.apply_plans(cpu_floats, plans, (224, 224), saltiness=0.02, spiciness=0.02)
    assert (got - exp).abs().max().item() < 1e-4


@pytest.mark.parametrize("layout", [HWC, CHW])
def test_wide_window_in_column_chunks(layout):
    """A 12 x 5000 image resized whole to 224 wide: its rows do not fit the staged row, so the raw pass works in column
    chunks (and the f32 plane it writes is read back as an F32 source by the crop)."""
    from ebc_amd.transforms import CropAugment, CropPlan
    aug = CropAugment(16, jitter_prob=0.0, blur_prob=0.0, noise_prob=0.0)
    img = _u8(12, 5000, 21)
    plans = [CropPlan(0, 0, 0, 16, 224, (16, 224), False), CropPlan(0, 0, 100, 16, 124, (16, 224), True),
             CropPlan(0, 0, 0, 12, 5000, None, False), CropPlan(0, 0, 3, 12, 4997, None, True),
             CropPlan(1, 0, 0, 12, 5000, None, False)]      # from the f32 image: one column's taps pass a staged row
    f = _f32(img)
    want = aug.apply([f, f], plans, normalize=False).cpu()
    raw = _as(img, layout)
    assert torch.equal(aug.apply([raw.cuda(), f], plans, normalize=False).cpu(), want)
    assert torch.equal(aug.apply([raw, f], plans, normalize=False).cpu(), want)


@pytest.mark.parametrize("noise_rng", ["device", "reference"])
def test_full_pipeline_stream_is_the_float_streams(noise_rng):
    """Every op at probability 1 with hue: `__call__` on raw sources (sizes taken from the layout) gives the float
    sources' batch bit for bit and leaves the CPU generator in the same state."""
    from ebc_amd.transforms import CropAugment
    shapes = [(300, 401), (150, 180), (230, 261)]
    imgs = [_u8(h, w, 30 + i) for i, (h, w) in enumerate(shapes)]
    g = torch.Generator().manual_seed(2)
    labs = [torch.rand(30, 2, generator=g) * torch.tensor([w, h], dtype=torch.float32) for h, w in shapes]
    aug = CropAugment(224, 1.0, 2.0, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, saltiness=0.02,
                      spiciness=0.02, jitter_prob=1.0, blur_prob=1.0, noise_prob=1.0, noise_rng=noise_rng)
    torch.manual_seed(41)
    want = aug([_f32(x) for x in imgs], labs, num_crops=2)
    nxt_want = torch.rand(1).item()
    raws = [_as(imgs[0], HWC).cuda(), _as(imgs[1], CHW), _as(imgs[2], HWC)]
    torch.manual_seed(41)
    got = aug(raws, labs, num_crops=2)
    assert torch.rand(1).item() == nxt_want
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))


LOADER_SHAPES = [(40, 52), (64, 45), (33, 70), (25, 30), (48, 48)]


def _loader_data():
    imgs = [_u8(h, w, 50 + i) for i, (h, w) in enumerate(LOADER_SHAPES)]
    g = torch.Generator().manual_seed(8)
    labs = [torch.rand(12, 2, generator=g) * torch.tensor([w, h], dtype=torch.float32) for h, w in LOADER_SHAPES]
    stored = [_as(x, HWC if i % 2 == 0 else CHW) for i, x in enumerate(imgs)]
    return imgs, stored, labs


def test_loader_modes_agree_and_equal_call():
    """5 images, batch 2, 2 crops: resident x prefetch give identical batches over two epochs (the pinned buffers are
    reused at other sizes in the second), the last batch is short, and the batches are `CropAugment.__call__`'s on the
    float images in the sampler's order under the same seed."""
    from torch.utils.data import DistributedSampler
    from ebc_amd.loader import RawCropLoader
    from ebc_amd.transforms import CropAugment
    imgs, stored, labs = _loader_data()
    aug = CropAugment(32, 1.0, 2.0, brightness=0.4, contrast=0.4, saturation=0.4, saltiness=0.02, spiciness=0.02,
                      jitter_prob=0.5, blur_prob=0.5, noise_prob=0.5)
    floats = [_f32(x) for x in imgs]
    sampler = DistributedSampler(range(5), num_replicas=1, rank=0, shuffle=True, seed=4)
    want = []
    torch.manual_seed(77)
    for epoch in (0, 1):
        sampler.set_epoch(epoch)
        idx = list(sampler)
        for b in range(0, 5, 2):
            batch = idx[b:b + 2]
            want.append(aug([floats[k] for k in batch], [labs[k] for k in batch], num_crops=2))
    assert [w[0].shape[0] for w in want] == [4, 4, 2, 4, 4, 2]
    for resident in (True, False):
        for prefetch in (True, False):
            loader = RawCropLoader(stored, labs, aug, batch_size=2, num_crops=2, shuffle=True, seed=4,
                                   resident=resident, prefetch=prefetch)
            assert len(loader) == 3
            got = []
            torch.manual_seed(77)
            for epoch in (0, 1):
                loader.set_epoch(epoch)
                for image, points, density in loader:
                    # what a training step does with the batch while the next one is on its way
                    got.append((image.clone(), points, density.clone()))
            torch.cuda.synchronize()
            assert len(got) == len(want) == 6
            for k, (g, w) in enumerate(zip(got, want)):
                assert g[0].is_cuda and g[0].dtype == torch.float32 and g[0].shape == w[0].shape, (resident, prefetch, k)
                assert torch.equal(g[0], w[0]), (resident, prefetch, k)
                assert torch.equal(g[2], w[2]), (resident, prefetch, k)
                assert len(g[1]) == len(w[1]) and all(torch.equal(a, b) for a, b in zip(g[1], w[1]))


def test_training_epoch_over_the_loader():
    """One `ebc_amd.train.train` epoch (2-layer clip_vit_b_16, 4 crops a step, fp16 autocast) over a RawCropLoader."""
    from ebc_amd.loader import RawCropLoader
    from ebc_amd.losses import DACELoss
    from ebc_amd.model import get_model
    from ebc_amd.train import train
    from ebc_amd.transforms import CropAugment
    shapes = [(300, 401), (260, 330), (150, 180), (240, 250)]
    imgs = [_as(_u8(h, w, 60 + i), HWC if i % 2 else CHW) for i, (h, w) in enumerate(shapes)]
    g = torch.Generator().manual_seed(9)
    labs = [torch.rand(40, 2, generator=g) * torch.tensor([w, h], dtype=torch.float32) for h, w in shapes]
    txt = torch.from_numpy(golden("f6_text.npz")["text_features_word"])
    model = get_model("clip_vit_b_16", 224, 8, BINS, ANCHORS_NWPU, prompt_type="word", vit_layers=2, weights_seed=0,
                      text_features=txt).cuda()
    loss_fn = DACELoss(BINS, 8, weight_count_loss=1.0, count_loss="dmcount", input_size=224)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    scaler = torch.amp.GradScaler("cuda")
    torch.manual_seed(3)
    loader = RawCropLoader(imgs, labs, CropAugment(224), batch_size=2, num_crops=2, seed=1)
    _, _, _, info = train(model, loader, loss_fn, opt, scaler, torch.device("cuda"), 0, 1, progress=False)
    assert info and all(torch.isfinite(torch.tensor(v)) for v in info.values()), info
