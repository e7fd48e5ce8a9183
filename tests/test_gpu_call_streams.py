"""-m gpu: the training ops launch on torch's CURRENT stream of their tensors' device, whichever device is current -- what _C.launch
(diff_gaussian_rasterization_ch3/_C.py) gives every one of them.  Each of fused_adam, fused_loss, fused_epilogue, fused_mlp and fused_hexplane,
at the smallest case of its own GPU test, under a side stream: every stream handle the binding hands to the library is the side stream's,
and outputs and gradients are bit-equal to the same call on the default stream."""
import numpy as np
import pytest
import torch


def _leaf(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).requires_grad_(True)


def _adam(dev):                 # tests/test_adam.py: P = 1, the seven groups of the model
    import fused_adam
    rng = np.random.default_rng(2)
    shapes = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "temporal_pos": (1,)}
    ps = {k: _leaf(rng.normal(size=(1,) + s), dev) for k, s in shapes.items()}
    opt = fused_adam.GaussianAdam([{"params": [p], "lr": 1e-3, "name": k} for k, p in ps.items()], eps=1e-15)
    for _ in range(2):
        for p in ps.values():
            p.grad = torch.from_numpy(rng.normal(size=tuple(p.shape)).astype(np.float32)).to(dev)
        opt.step()
    return [t for p in ps.values() for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]


def _loss(dev):                 # tests/test_loss.py: a [1, 1, 1] image
    import fused_loss
    img, gt = _leaf([[[0.25]]], dev), torch.tensor([[[0.75]]], device=dev)
    loss, parts = fused_loss.l1_dssim_loss(img, gt, 0.2, return_parts=True)
    (3.0 * loss).backward()
    return [loss.detach(), parts, img.grad]


def _epilogue(dev):             # tests/test_epilogue.py: P = 1, M = 1, every residual
    import fused_epilogue
    rng = np.random.default_rng(33)
    t = {k: _leaf(rng.normal(size=s), dev) for k, s in dict(xyz=(1, 3), rotation=(1, 4), scaling=(1, 3), opacity=(1, 1), f_dc=(1, 1, 3), f_rest=(1, 0, 3),
                                                             motion_res=(1, 3), rot_res=(1, 7), trbf=(1, 1), shs_res=(1, 1, 3)).items()}
    outs = fused_epilogue.activate_gaussians(t["xyz"], t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"], motion_residual=t["motion_res"],
                                             rot_residual=t["rot_res"], trbfoutput=t["trbf"], shs_residual=t["shs_res"])
    torch.autograd.backward(outs, [torch.from_numpy(rng.normal(size=tuple(o.shape)).astype(np.float32)).to(dev) for o in outs])
    return [o.detach() for o in outs] + [v.grad for v in t.values()]


def _mlp(dev):                  # tests/test_gpu_mlp.py: CORNERS[0] = 1 -> 32 -> 32 -> 1, one row
    import fused_mlp
    import mlp_math as mm
    c = mm.make_case(1, 0, 32, 32, 1, 1)
    t = {k: _leaf(c[k], dev) for k in ("x", "w1", "b1", "w2", "b2", "w3", "b3")}
    y = fused_mlp.fused_mlp3(*t.values())
    y.backward(torch.from_numpy(c["dy"]).to(dev))
    return [y.detach()] + [v.grad for v in t.values()]


def _hexplane(dev):             # tests/test_hexplane.py: test_row_counts' 16 x 16 plane, C = 4, N = 1
    import fused_hexplane
    rng = np.random.default_rng(77 * 4 + 1)
    g, p, lv = _leaf(rng.normal(size=(1, 4, 16, 16)), dev), _leaf(rng.uniform(0.0, 1.0, size=(1, 2)), dev), _leaf([[1.25, 2.5]], dev)
    o = fused_hexplane.texture_planes(p, lv, [g], [(0, 1)], [7], [0], 4)
    o.backward(torch.from_numpy(rng.normal(size=(1, 4)).astype(np.float32)).to(dev))
    return [o.detach(), g.grad, p.grad, lv.grad]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["current_device", "other_device"])
@pytest.mark.parametrize("run", [_adam, _loss, _epilogue, _mlp, _hexplane], ids=lambda f: f.__name__[1:])
def test_training_ops_launch_on_the_current_stream_of_their_device(run, where, rast, gpu, monkeypatch):
    _C = rast._C
    dev = gpu
    if where == "other_device":             # the tensors on device 1 while device 0 is current
        if torch.cuda.device_count() < 2:
            pytest.skip("one device visible")
        dev = torch.device("cuda:1")
    seen, real = [], _C._stream_of

    def recording(d):
        seen.append((d, real(d)))
        return seen[-1][1]
    monkeypatch.setattr(_C, "_stream_of", recording)
    with torch.cuda.device(gpu):
        want = run(dev)
        torch.cuda.synchronize(dev)
        assert seen and all(d == dev and h == torch.cuda.default_stream(dev).cuda_stream for d, h in seen)
        del seen[:]
        side = torch.cuda.Stream(device=dev)
        assert side.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.cuda.device(gpu):      # (entering a stream of another device makes that device current: back to `gpu`)
            assert torch.cuda.current_device() == gpu.index
            got = run(dev)
        side.synchronize()
    assert seen and all(d == dev and h == side.cuda_stream for d, h in seen), seen
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.device == dev and torch.equal(a, b), k
