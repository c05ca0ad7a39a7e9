"""CPU pins of tests/_optim_refs.py: the float64 step against torch.optim.Adam on float64 tensors, the scaler function
against torch.amp.GradScaler on the CPU, the f32 stand-in inside every bound, and each corruption the GPU module
(tests/test_gpu_optim_kernels.py) has to catch pushing a ratio above 1 (or flipping a flag) on that module's own cases."""
import numpy as np
import pytest
import torch

import _optim_refs as OR

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("name,h", [("wd0", OR.Hyper(wd=0.0)), ("wd", OR.Hyper(wd=1e-2)),
                                    ("betas", OR.Hyper(beta1=0.8, beta2=0.95, eps=1e-6, wd=1e-4))])
def test_adam_f64_is_torch_adam(name, h):
    g = np.random.Generator(np.random.PCG64(3))
    p = g.standard_normal(257)
    m, v = np.zeros(257), np.zeros(257)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=h.wd)
    for step in range(5):
        gr = g.standard_normal(257)
        tp.grad = torch.from_numpy(gr.copy())
        opt.step()
        r = OR.adam_f64(p, gr, m, v, step, h)
        p, m, v = r["p1"], r["m1"], r["v1"]
        st = opt.state[tp]
        for ours, theirs in ((p, tp.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            t = theirs.numpy()
            assert np.abs(ours - t).max() <= 1e-12 * np.abs(t).max(), (name, step)


def _torch_scaler_sequence(h, scale0, skips, steps):
    if hasattr(torch.amp, "GradScaler"):
        try:
            sc = torch.amp.GradScaler("cpu", init_scale=scale0, growth_factor=h.growth, backoff_factor=h.backoff,
                                      growth_interval=h.interval)
            p = torch.nn.Parameter(torch.zeros(1))
            opt = torch.optim.SGD([p], lr=0.0)
            out = []
            for i in range(steps):
                sc.scale(torch.ones(()))
                p.grad = torch.tensor([float("inf") if i in skips else 1.0])
                sc.step(opt)
                sc.update()
                out.append((float(sc.get_scale()), int(sc._growth_tracker)))
            return out
        except (RuntimeError, AssertionError, TypeError):
            pass
    s, t = torch.tensor(scale0, dtype=torch.float32), torch.tensor(0, dtype=torch.int32)
    out = []
    for i in range(steps):
        torch._amp_update_scale_(s, t, torch.tensor(1.0 if i in skips else 0.0), h.growth, h.backoff, h.interval)
        out.append((float(s), int(t)))
    return out


SEQUENCES = [("issue", 2.0 ** 127, {2, 7}), ("refused", 1.5 * 2.0 ** 127, {7}), ("small", 3.0, {0, 1, 5})]


def scaler_sequence(fn, h, scale0, skips, steps=12, **kw):
    s, t, k = F32(scale0), F32(0), F32(0)
    out = []
    for i in range(steps):
        s, t, f, k = fn(s, t, i in skips, k, h, **kw)
        out.append((float(s), int(t), float(f), float(k)))
    return out


@pytest.mark.parametrize("name,scale0,skips", SEQUENCES)
def test_scaler_next_is_torch_grad_scaler(name, scale0, skips):
    h = OR.Hyper(growth=1.5, backoff=0.25, interval=3)
    ours = scaler_sequence(OR.scaler_next, h, scale0, skips)
    assert [(s, t) for s, t, _, _ in ours] == _torch_scaler_sequence(h, scale0, skips, 12)
    applied = np.cumsum([i not in skips for i in range(12)])
    assert [k for _, _, _, k in ours] == list(applied.astype(float))           # the count of applied steps
    if name == "refused":                   # a growth that would overflow: the scale stays, the tracker resets
        assert ours[1][:2] == (scale0, 2) and ours[2][:2] == (scale0, 0) and float(F32(scale0)) * 1.5 > float(np.finfo(F32).max)
    assert scaler_sequence(OR.scaler_standin, h, scale0, skips) == ours


def _runs():
    """Every (hyper, mode, first step) of the GPU module on a short tensor list."""
    for hi, (hn, h) in enumerate(OR.HYPERS.items()):
        for mi, (mn, (scale, wg)) in enumerate(OR.MODES.items()):
            yield hn, mn, h, scale, wg, OR.STEPS0[(hi + mi) % 3]


def _worst(bug=None):
    """Largest ratio per output kind over the runs, three steps each, the stand-in in the kernel's place; and whether
    a gradient buffer that must keep its bits lost them."""
    worst, grad_kept = {}, True
    for hn, mn, h, scale, wg, step0 in _runs():
        for n in (5, 1023):
            p, m, v = OR.tensor_inputs(n, 100 + n)
            for k in range(3):
                g = OR.grad_inputs(n, 7 * n + k, scale)
                before = (p, g, m, v)
                after = OR.step_standin(p, g, m, v, step0 + k, h, scale, wg, bug=bug)
                for kind, (e, b) in OR.step_ratios(before, after, step0 + k, h, scale, wg).items():
                    worst[kind] = max(worst.get(kind, 0.0), OR.ratio(e, b))
                if scale is None or not wg:
                    grad_kept &= after[1].tobytes() == g.tobytes()
                if h.lr == 0.0:
                    assert bug is not None or after[0].tobytes() == p.tobytes()
                p, _, m, v = after
    return worst, grad_kept


def test_standin_is_inside_every_bound():
    worst, grad_kept = _worst()
    print({k: round(r, 4) for k, r in worst.items()})
    assert set(worst) == {"g", "m", "v", "p"} and all(r <= 1.0 for r in worst.values()), worst
    assert grad_kept


@pytest.mark.parametrize("bug,kind", [("bc_step", "p"), ("wd_after_m", "m"), ("eps_in_sqrt", "p")])
def test_update_corruptions_leave_the_bound(bug, kind):
    worst, _ = _worst(bug)
    print(bug, {k: round(r, 4) for k, r in worst.items()})
    assert worst[kind] > 1.0, (bug, worst)


def test_write_grad_corruption_changes_the_gradient_bits():
    assert _worst("write_grad_always")[1] is False


@pytest.mark.parametrize("bug,seq", [("step_on_skip", "issue"), ("no_reset_on_refused", "refused")])
def test_scaler_corruptions_leave_the_sequence(bug, seq):
    h = OR.Hyper(growth=1.5, backoff=0.25, interval=3)
    _, scale0, skips = next(s for s in SEQUENCES if s[0] == seq)
    assert scaler_sequence(OR.scaler_standin, h, scale0, skips, bug=bug) != scaler_sequence(OR.scaler_next, h, scale0, skips)
    if bug == "no_reset_on_refused":        # the 12 steps from 2^127 alone refuse no growth: they do not see this one
        _, s0, sk = SEQUENCES[0]
        assert scaler_sequence(OR.scaler_standin, h, s0, sk, bug=bug) == scaler_sequence(OR.scaler_next, h, s0, sk)


def _check_cases(bug=None):
    """The GPU module's inf-check calls on the stand-in: (size, layout, position or None) -> the flag it would set.
    Around the gradient lie NaN frame elements, as in the no-false-positive calls."""
    wrong = []
    for n in OR.SIZES:
        for layout in OR.LAYOUTS:
            aligned = layout == "aligned"
            ext = np.full(n + 8, np.nan, F32)
            clean = OR.clean_edge_grad(n, n)
            assert np.isfinite(clean).all()
            ext[4:4 + n] = clean
            if OR.check_standin(ext, 4, n, aligned, bug):
                wrong.append((n, layout, None))
            for k, pos in enumerate(OR.check_positions(n, aligned)):
                ext[4:4 + n] = clean
                ext[4 + pos] = OR.BAD[k % 3]
                if not OR.check_standin(ext, 4, n, aligned, bug):
                    wrong.append((n, layout, pos))
    return wrong


def test_check_cases_and_their_corruptions():
    assert _check_cases() == []
    seen = {bug: _check_cases(bug) for bug in ("skip_remainder", "drop_piece3", "wave0_only", "n4_up")}
    for bug, wrong in seen.items():
        print(bug, wrong[:6])
        assert wrong and all(layout == "aligned" or bug == "wave0_only" for _, layout, _ in wrong), bug
    assert (5123, "aligned", 5120) in seen["skip_remainder"] and (4097, "aligned", 4096) in seen["skip_remainder"]
    assert (4096, "aligned", 4 * (192 + 768) + 0) in seen["drop_piece3"]
    assert (4096, "aligned", 4 * (64 + 256) + 2) in seen["wave0_only"]
    assert all(pos is None for _, _, pos in seen["n4_up"])         # a read past numel: the NaN frame raises the flag


def test_check_positions_reach_every_path():
    for n in OR.SIZES:
        pos = OR.check_positions(n, True)
        assert pos[0] == 0 and pos[-1] == n - 1 and len(set(pos)) == len(pos) and all(0 <= q < n for q in pos)
    assert {4095, 4096, 5119, 5120, 5121, 5122} <= set(OR.check_positions(5123, True))
    owners = {((q // 4) % 256) // 64: (q // 4) // 256 for q in OR.check_positions(4096, True) if 0 < q < 4095}
    assert owners == {0: 0, 1: 1, 2: 2, 3: 3}                      # wave -> unrolled piece
