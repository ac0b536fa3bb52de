"""GPU tests of the PyTorch-ROCm network on HIP-voxelized input and of bench.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_on_gpu_matches_golden(gpu):
    import torch
    import pp_amd.model as M
    g = np.load(os.path.join(ROOT, "tests", "golden", "model_golden.npz"))
    canvas, c, p, n, a_per = [int(v) for v in g["dims"]]
    net = M.PPModel(9, c, a_per * 9, a_per * 8, canvas, canvas)
    net.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")})
    net = net.to(gpu).eval()
    with torch.no_grad():
        cl, rg = net(torch.from_numpy(g["pillars"]).to(gpu), torch.from_numpy(g["inds"]).to(gpu))
    assert np.abs(cl.cpu().numpy() - g["cls_eval"]).max() < 1e-4      # f32 conv, different summation order
    assert np.abs(rg.cpu().numpy() - g["reg_eval"]).max() < 1e-4


def test_pipeline_forward_equals_model_on_oracle_pillars(gpu, oracle):
    """End to end: HIP voxelizer + network == network on the oracle's voxel stage."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    from util import oracle_stage
    cfg = VoxelConfig.square(16.0, 0.2, 4000, 32)
    pipe = PillarPipeline(cfg, feature_channels=16, device=gpu, seed=0)
    pipe.model.eval()
    pts = synth.lidar_like(15000, 16.0, 3)
    cl, rg = pipe.forward(torch.from_numpy(pts).to(gpu))
    ref_p, ref_i, _ = oracle_stage(oracle, pts, 4000, 32, 16.0, 0.2, order=cfg.order)
    with torch.no_grad():
        cl2, rg2 = pipe.model(torch.from_numpy(ref_p)[None].to(gpu), torch.from_numpy(ref_i)[None].to(gpu))
    assert cl.shape == (1, 18, 80, 80) and rg.shape == (1, 16, 80, 80)
    assert torch.equal(cl, cl2) and torch.equal(rg, rg2)


def test_train_step_runs_and_is_finite(gpu):
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(16.0, 0.2, 3000, 16)
    pipe = PillarPipeline(cfg, feature_channels=8, device=gpu, seed=0, with_targets=True)
    pipe.model.train()
    pts = torch.from_numpy(np.stack([synth.lidar_like(12000, 16.0, s) for s in (0, 1)])).to(gpu)
    gts = [synth.gt_boxes(6, 160, s, margin=25.0) for s in (0, 1)]
    cl, rl, ol, tot = pipe.train_forward_backward(pts, gts)
    assert all(torch.isfinite(v) for v in (cl, rl, ol, tot))
    grads = [p.grad for p in pipe.model.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)


def test_bench_contract_line(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--no-stress", "--no-train-leg"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["value"] > 0 and j["vs_baseline"] is None
    rf = j["roofline"]
    assert rf["bound"] == "hbm" and 0 < rf["frac"] < 1
    # the headline's voxelizer is the software-pipelined one: ONE kernel (k_step) whose fraction is the whole
    # voxelizer's; the three-launch path is measured beside it
    assert rf["kernel"].startswith("pp::k_step") and rf["pipeline_frac"] == rf["frac"]
    assert set(rf["three_launch"]["kernels_us"]) == {"k_split", "k_tile", "k_emit"}
    # roofline.traffic: measured in the run itself (two rocprofv3 --pmc child runs of the headline loop) where the
    # profiler is available; the committed constant otherwise, and labelled so
    if "traffic_detail" in rf:
        assert rf["traffic_source"].startswith("measured in this run")
        assert rf["bytes_per_launch"] * 0.95 < rf["traffic"] < rf["bytes_per_launch"] * 1.35
        assert abs(rf["traffic"] - rf["traffic_static"]) < 0.08 * rf["traffic_static"]
        assert min(rf["traffic_detail"]["launches"]) >= 4
    else:
        assert rf["traffic"] is None or rf["traffic_source"].startswith("static")
    assert 0 < rf["three_launch"]["pipeline_frac"] < rf["three_launch"]["k_emit_frac"] < 1
    vo = j["voxelizer_only"]
    for rec in (vo, vo["row_major_order"], vo["one_sweep_per_launch"], vo["c1_shapes"]):
        assert 0 < rec["wall_frac"] < 1 and rec["k_step_us"] > 0 and 0 < rec["three_launch"]["wall_frac"] < 1
    fr = j["fused_feature_net"]["roofline"]
    assert fr["bytes_per_launch"] > 0 and 0 < fr["frac"] < 1 and set(fr["kernels_us"]) == {"k_split", "k_tile", "k_emit"}
    # the rows either side of the path and the drop-in surface's own speed, in the same line
    nr = j["next_rows"]
    assert nr["ingest"]["us_per_sample"] > 0 and nr["ingest"]["bytes_per_launch"] == 5 * 60000 * 36
    pp_ = nr["postprocess"]
    assert pp_["samples"] == 4 and pp_["us_per_batch"] > 0 and all(200 < c < 5000 for c in pp_["candidates_per_sample"])
    assert all(0 < k <= 100 for k in pp_["kept_per_sample"])
    dh = j["dropin_host"]
    for leg in ("create_pillars_call", "create_pillars_in_dataset_glue", "make_ious_call"):
        r = dh[leg]
        assert r["hip_ms"] > 0 and r["cpu_ms"] > 0 and abs(r["speedup"] - r["cpu_ms"] / r["hip_ms"]) < 1e-9
        assert r["meets_50x"] == (r["speedup"] >= 50.0)
        assert r["faithful_cpu_ms"] > 0 and abs(r["faithful_speedup"] - r["faithful_cpu_ms"] / r["hip_ms"]) < 1e-9
    fa = dh["create_pillars_call"]["fresh_arrays"]
    assert fa["hip_ms"] > 0 and fa["cpu_ms"] > fa["hip_ms"] and abs(fa["speedup"] - fa["cpu_ms"] / fa["hip_ms"]) < 0.02
    # make_ious with the anchors resident (the reference's call pattern) and with one anchor edited before every call
    mi = dh["make_ious_call"]
    assert mi["anchors_changed_every_call_ms"] >= mi["hip_ms"] * 0.9
    assert abs(mi["anchors_changed_every_call_speedup"] - mi["cpu_ms"] / mi["anchors_changed_every_call_ms"]) < 0.02


def test_bench_plain_line_and_dumped_outputs(gpu, tmp_path):
    """A plain run (no --full): the contract line with the headline's roofline and none of the side legs; and
    --dump-outputs writes the (cls, reg) the last timed step handed back, equal to a forward of that step's batch."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "sweeps/s" and j["dtype"] == "f32"
    assert abs(j["value"] - 3 * 4 / (j["ms_per_step"] * 3e-3)) < 1e-6 * j["value"]
    assert j["roofline"]["kernel"].startswith("pp::k_step") and "three_launch" not in j["roofline"]
    for k in ("overlapped", "voxelizer_only", "fused_feature_net", "train_c3", "stress_c5", "reference_default",
              "next_rows", "dropin_host", "cpu_baseline"):
        assert k not in j, k
    assert sorted(os.listdir(d)) == ["cls.npy", "reg.npy"]
    cl, rg = np.load(d / "cls.npy"), np.load(d / "reg.npy")
    assert cl.dtype == rg.dtype == np.float32 and cl.shape == (4, 18, 250, 250) and rg.shape == (4, 16, 250, 250)
    # the step's batch: the pipelined call k uses resident set k % 4 and returns the batch of call k - LAG; with
    # warm-up 1 (+ LAG filling calls) and 3 timed steps the last timed step returns set (1 + 3) % 4 = 0, seeds 0..3
    pipe = PillarPipeline(VoxelConfig.square(50.0, 0.2, 12000, 100), device=gpu, seed=0)
    pipe.model.eval()
    pts = torch.from_numpy(np.stack([synth.lidar_like(60000, 50.0, s) for s in range(4)])).to(gpu)
    c_ref, r_ref = (t.cpu().numpy() for t in pipe.forward(pts))
    for got, ref in ((cl, c_ref), (rg, r_ref)):
        assert np.abs(got - ref).max() <= 2e-3 * max(1.0, float(np.abs(ref).max()))


def test_fused_epilogue_equals_relu_batchnorm(gpu):
    """Backbone in eval mode: conv + fused bias/ReLU/BN kernel == Conv2d -> ReLU -> BatchNorm2d."""
    import torch
    import pp_amd.model as M
    torch.manual_seed(5)
    bb = M.PPBackbone(16, up3_op=M.up3_output_padding(96)).to(gpu)
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.4, 2.0)
                m.weight.normal_(0, 1.0)
                m.bias.normal_(0, 0.2)
    bb.eval()
    x = torch.randn(2, 16, 96, 96, device=gpu)
    with torch.no_grad():
        y1 = bb(x)
        for m in bb.modules():
            if hasattr(m, "fused_epilogue"):
                m.fused_epilogue = False
        y0 = bb(x)
    assert y1.shape == y0.shape == (2, 96, 48, 48)
    assert (y1 - y0).abs().max().item() <= 2e-4 * max(1.0, y0.abs().max().item())
    # odd spatial size: scalar tail / unaligned planes
    d = M.PPDownBlock(2, 3, 5).to(gpu).eval()
    xx = torch.randn(1, 3, 37, 41, device=gpu)
    with torch.no_grad():
        a = d(xx)
        d.fused_epilogue = False
        b = d(xx)
    assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)


def test_channels_last_backbone_equals_nchw(gpu):
    """The inference backbone + merged head on a channels-last canvas (MIOpen NHWC kernels,
    the NHWC epilogue writing channel slices of the concatenated output) == the NCHW path
    == plain Conv2d -> ReLU -> BatchNorm2d modules."""
    import torch
    import pp_amd.model as M
    torch.manual_seed(7)
    bb = M.PPBackbone(16, up3_op=M.up3_output_padding(100)).to(gpu)
    head = M.PPDetectionHead(96, 18, 16).to(gpu)
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.4, 2.0)
                m.weight.normal_(0, 1.0)
                m.bias.normal_(0, 0.2)
    bb.eval()
    head.eval()
    x = torch.randn(3, 16, 100, 100, device=gpu)
    with torch.no_grad():
        y_nchw = bb(x)
        c_nchw, r_nchw = head(y_nchw)
        y_cl = bb(x.contiguous(memory_format=torch.channels_last))
        c_cl, r_cl = head(y_cl)
        for m in bb.modules():
            if hasattr(m, "fused_epilogue"):
                m.fused_epilogue = False
        y_ref = bb(x)
        c_ref, r_ref = head(y_ref)
    assert y_cl.shape == y_ref.shape == (3, 96, 50, 50)
    assert y_cl.is_contiguous(memory_format=torch.channels_last)
    tol = 2e-4 * max(1.0, y_ref.abs().max().item())
    assert (y_cl - y_ref).abs().max().item() <= tol
    assert (y_nchw - y_ref).abs().max().item() <= tol
    for a, b in ((c_cl, c_ref), (r_cl, r_ref), (c_nchw, c_ref), (r_nchw, r_ref)):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 2e-4 * max(1.0, b.abs().max().item())
    # channel counts that are not multiples of 4 fall back to the NCHW kernel
    d = M.PPDownBlock(2, 3, 5).to(gpu).eval()
    xx = torch.randn(1, 3, 37, 41, device=gpu)
    with torch.no_grad():
        a = d(xx.contiguous(memory_format=torch.channels_last))
        d.fused_epilogue = False
        b = d(xx)
    assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)


def test_fused_relu_batchnorm_training_matches_autograd(gpu):
    """bn(relu(z)) in train() through the fused HIP kernels (forward: batch statistics, running
    statistics, output; backward: dz, dgamma, dbeta) against PyTorch's modules + autograd in
    f64.  Shapes: vector path, odd planes (scalar path), one slice, many slices."""
    import torch
    import pp_amd.model as M
    for shape in ((4, 64, 60, 60), (2, 5, 63, 63), (1, 3, 7, 5), (3, 16, 250, 250)):
        res = {}
        for name, dtype, fused in (("f64", torch.float64, False), ("t32", torch.float32, False),
                                   ("hip", torch.float32, True)):
            torch.manual_seed(3)
            bn = torch.nn.BatchNorm2d(shape[1]).to(gpu)
            with torch.no_grad():
                bn.weight.normal_(0, 1.0)
                bn.bias.normal_(0, 0.5)
                bn.running_mean.normal_(0, 0.2)
                bn.running_var.uniform_(0.5, 1.5)
            bn = bn.to(dtype).train()
            g = torch.Generator(device="cpu").manual_seed(1)
            z = (torch.randn(shape, generator=g) * 1.5 + 0.2).to(gpu).to(dtype).requires_grad_(True)
            dy = torch.randn(shape, generator=g).to(gpu).to(dtype)
            cb = None
            if shape[1] != 5:      # with the convolution bias folded in (and its gradient out)
                cb = (torch.randn(shape[1], generator=g) * 0.5).to(gpu).to(dtype).requires_grad_(True)
            y = M._relu_bn(z, bn, enabled=fused, conv_bias=cb)
            if shape[1] == 16:     # gradient arriving as a channel slice of a wider tensor (torch.cat)
                wide = torch.zeros(shape[0], shape[1] + 8, *shape[2:], device=gpu, dtype=dtype)
                wide[:, 4:4 + shape[1]] = dy
                y.backward(wide[:, 4:4 + shape[1]])
            else:
                y.backward(dy)
            res[name] = dict(y=y.detach().double(), dz=z.grad.double(), dg=bn.weight.grad.double(),
                             dcb=(cb.grad.double() if cb is not None else torch.zeros(1, device=gpu).double()),
                             db=bn.bias.grad.double(), rm=bn.running_mean.double(), rv=bn.running_var.double(),
                             nb=int(bn.num_batches_tracked))
        torch.cuda.synchronize()
        assert res["hip"]["nb"] == 1
        for key in ("y", "dz", "dg", "db", "dcb", "rm", "rv"):
            ref = res["f64"][key]
            scale = ref.abs().max().clamp(min=1e-30)
            e_hip = ((res["hip"][key] - ref).abs().max() / scale).item()
            e_t32 = ((res["t32"][key] - ref).abs().max() / scale).item()
            assert e_hip <= 1e-5 + 4 * e_t32, (shape, key, e_hip, e_t32)


def test_training_steps_reduce_the_loss(gpu):
    """End-to-end sanity of the HIP training path (voxelizer -> on-the-fly anchors / targets ->
    HIP feature net + fused ReLU/BatchNorm kernels -> loss -> backward): a few Adam steps on
    one fixed batch lower the total loss, everything stays finite, running statistics move."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(16.0, 0.2, 3000, 32)
    pipe = PillarPipeline(cfg, device=gpu, seed=0, with_targets=True)
    pipe.model.train()
    pts = torch.from_numpy(np.stack([synth.lidar_like(12000, 16.0, s) for s in (0, 1)])).to(gpu)
    gts = [pipe.upload_ground_truth(synth.gt_boxes(12, cfg.canvas_height, s)) for s in (0, 1)]
    opt = torch.optim.Adam(pipe.model.parameters(), lr=2e-3)
    rv0 = pipe.model.backbone.down1.block[2].running_var.clone()
    totals = []
    for _ in range(12):
        opt.zero_grad(set_to_none=True)
        losses = pipe.train_forward_backward(pts, gts)
        totals.append(losses[3].item())
        assert all(torch.isfinite(t).all() for t in losses)
        opt.step()
    assert totals[-1] < 0.8 * totals[0], totals
    assert not torch.equal(rv0, pipe.model.backbone.down1.block[2].running_var)
    assert int(pipe.model.feature_net.bn1.num_batches_tracked) == 12


def test_inference_chain_raw_rows_to_boxes(gpu, oracle):
    """The whole device-resident inference chain of INTEGRATION.md section 3: raw .bin rows ->
    pp_ingest_dev -> fused voxelizer / feature net / scatter -> backbone + head (channels last)
    -> pp_decode_strided_dev on the channel slices.  The fused + strided chain must give exactly
    the boxes of the dense, copy-based chain fed to the oracle's post-processing."""
    import torch
    from pp_amd import boxes, synth
    from pp_amd.ingest import LidarIngest
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.postprocess import Detector
    from pp_amd.voxelizer import VoxelConfig
    half, step = 16.0, 0.2
    cfg = VoxelConfig.square(half, step, 4000, 32)
    pipe = PillarPipeline(cfg, device=gpu, seed=3)
    pipe.model.eval()
    with torch.no_grad():      # make some anchors fire
        pipe.model.det_head.cls.bias.fill_(-0.6)
    acfg = pipe.anchor_cfg
    anchors = boxes.make_anchors(acfg)
    H = cfg.canvas_height
    det = Detector(anchors, acfg, H, step, step, -half, -half, pos_thresh=0.3, nms_thresh=0.1, device=gpu)
    raw = np.concatenate([synth.lidar_like(9000, half, 5), np.zeros((9000, 1), np.float32)], 1)   # 5 columns
    pose = np.eye(4)
    pose[:3, 3] = [0.5, -0.25, 0.1]
    pts = LidarIngest(device=gpu)([(raw, pose), (raw[:3000] * np.float32(0.5), np.eye(4))]).unsqueeze(0)
    cls_f, reg_f = pipe.forward_fused(pts)
    assert cls_f.stride(1) == 1                                   # channel slices of the merged head
    b_f, k_f, n_f = det(cls_f[0], reg_f[0])                       # read in place
    pipe.fused_scatter = False
    pipe.model.scatter.channels_last_inference = False
    cls_d, reg_d = pipe.forward(pts)                              # dense tensor, NCHW throughout
    torch.cuda.synchronize()
    assert (cls_f - cls_d).abs().max().item() <= 1e-4 * max(1.0, cls_d.abs().max().item())
    ref_b, ref_k = oracle.postprocess(cls_f[0].contiguous().cpu().numpy(), reg_f[0].contiguous().cpu().numpy(),
                                      anchors["centers"], anchors["wlh"], anchors["yaw"], anchors["xy"], H,
                                      step, step, -half, -half, pos_thresh=0.3, nms_thresh=0.1)
    n = int(n_f.item())
    assert n == len(ref_k) and n > 0
    assert np.array_equal(k_f.cpu().numpy()[:n], ref_k.astype(np.int32))
    assert np.allclose(b_f.cpu().numpy()[:n], ref_b, rtol=1e-5, atol=1e-5)


def test_eval_mode_gradients_do_not_go_through_the_raw_pointer_kernels(gpu):
    """model.eval() with autograd ON (frozen-BN fine-tuning, saliency): the in-place epilogue /
    merged-head inference shortcuts must step aside, or the backward would differentiate a bare
    convolution.  Gradients must equal those of the plain modules."""
    import copy
    import torch
    import pp_amd.model as M
    torch.manual_seed(11)
    bb = M.PPBackbone(16, up3_op=M.up3_output_padding(64)).to(gpu).eval()
    head = M.PPDetectionHead(96, 18, 16).to(gpu).eval()
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(0, 1.0)
    ref_bb, ref_head = copy.deepcopy(bb), copy.deepcopy(head)
    for m in list(ref_bb.modules()) + list(ref_head.modules()):
        for flag in ("fused_epilogue", "merge_heads"):
            if hasattr(m, flag):
                setattr(m, flag, False)
    x = torch.randn(2, 16, 64, 64, device=gpu).contiguous(memory_format=torch.channels_last)

    def grads(b, h):
        xx = x.clone().requires_grad_(True)
        c, r = h(b(xx))
        (c.square().sum() + r.sum()).backward()
        return [xx.grad] + [p.grad for p in list(b.parameters()) + list(h.parameters())]

    got, want = grads(bb, head), grads(ref_bb, ref_head)
    assert all(g is not None for g in got)        # conv bias, BN affine and both heads get gradients
    for g, w in zip(got, want):
        assert torch.allclose(g, w, rtol=1e-4, atol=1e-5 * max(1.0, w.abs().max().item()))
    with torch.no_grad():                          # and the shortcuts are still what inference runs
        c1, r1 = head(bb(x))
        c0, r0 = ref_head(ref_bb(x))
    assert (c1 - c0).abs().max().item() <= 2e-4 * max(1.0, c0.abs().max().item())


def test_fused_tables_follow_the_weights(gpu):
    """The fused feature-net table and the per-block epilogue tables are caches: after an
    optimizer step, a load_state_dict or a training forward (whose HIP kernels update the
    running statistics through raw pointers) inference must see the NEW values."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(12.0, 0.2, 2500, 32)
    pipe = PillarPipeline(cfg, device=gpu, seed=1, with_targets=True)
    pts = torch.from_numpy(synth.lidar_like(9000, 12.0, 2)).to(gpu).unsqueeze(0)

    def fused_vs_plain():
        pipe.model.eval()
        cf, rf = pipe.forward_fused(pts)
        flags = []
        for m in pipe.model.modules():             # the plain modules, no cache anywhere
            for f in ("fused_epilogue", "merge_heads", "hip_eval", "fast_eval", "channels_last_inference"):
                if hasattr(m, f):
                    flags.append((m, f, getattr(m, f)))
                    setattr(m, f, False)
        cd, rd = pipe.forward(pts)
        for m, f, v in flags:
            setattr(m, f, v)
        tol = 2e-4 * max(1.0, cd.abs().max().item())
        assert (cf - cd).abs().max().item() <= tol and (rf - rd).abs().max().item() <= tol
        return cf.clone()

    a = fused_vs_plain()
    # 1. a training step through the HIP training kernels + optimizer step
    opt = torch.optim.SGD(pipe.model.parameters(), lr=0.05)
    g = synth.gt_boxes(6, cfg.canvas_height, 0, margin=20.0)
    pipe.model.train()
    opt.zero_grad()
    pipe.train_forward_backward(pts, [g])
    opt.step()
    b = fused_vs_plain()
    assert (a - b).abs().max().item() > 0          # the step did change the network
    # 2. BatchNorm recalibration only: training-mode forwards under no_grad, parameters untouched
    pipe.model.train()
    with torch.no_grad():
        for _ in range(3):
            pipe.model(*pipe.voxelize(pts))
    c = fused_vs_plain()
    assert (b - c).abs().max().item() > 0
    # 3. load_state_dict
    sd = {k: (v * 1.05 if v.dtype.is_floating_point else v) for k, v in pipe.model.state_dict().items()}
    pipe.model.load_state_dict(sd)
    fused_vs_plain()


def test_forward_overlapped_equals_forward(gpu):
    """PillarPipeline.forward_overlapped (k_step on a side stream beside the network, two output buffers, events one
    step old): the same results as forward(), batch for batch, LAG + 1 calls later -- over changing clouds and batch
    sizes, with cache-flushing traffic on the main stream in between."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    pipe = PillarPipeline(VoxelConfig.square(16.0, 0.2, 4000, 32), feature_channels=64, device=gpu, seed=0)
    pipe.model.eval()
    clouds = [torch.from_numpy(np.stack([synth.lidar_like(n, 16.0, sd + s) for s in range(B)])).to(gpu)
              for n, sd, B in ((15000, 3, 2), (9000, 40, 2), (12000, 80, 1), (15000, 5, 3), (7000, 9, 2), (15000, 3, 2),
                               (11000, 60, 2))]
    want = [tuple(x.clone() for x in pipe.forward(c)) for c in clouds]
    torch.cuda.synchronize()
    junk = torch.empty(256 << 20, dtype=torch.uint8, device=gpu)
    outs = []
    lag = pipe.voxelizer.LAG + 1
    for k, c in enumerate(clouds + [None] * lag):
        r = pipe.forward_overlapped(c)
        assert (r is None) == (k < lag)
        if r is not None:
            outs.append(tuple(x.clone() for x in r))
        if k % 2 == 0:
            junk.zero_()
    torch.cuda.synchronize()
    assert len(outs) == len(clouds)
    for (c, r), (wc, wr) in zip(outs, want):
        assert c.shape == wc.shape
        assert (c - wc).abs().max().item() <= 2e-6 and (r - wr).abs().max().item() <= 2e-6


def test_forward_overlapped_orders_fresh_non_blocking_clouds(gpu):
    """clouds produced on the caller's stream right before the call (a non_blocking copy from pinned memory
    behind a long-running kernel) and dropped right after it.  The side stream must wait for the producer (an event
    recorded at entry) and hold the tensor's memory (record_stream) -- otherwise k_step voxelizes whatever the block
    held before, or what the next main-stream allocation writes into it."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    pipe = PillarPipeline(VoxelConfig.square(16.0, 0.2, 4000, 32), feature_channels=16, device=gpu, seed=0)
    pipe.model.eval()
    host = [torch.from_numpy(np.stack([synth.lidar_like(15000, 16.0, 10 * k + s) for s in range(2)])).pin_memory()
            for k in range(6)]
    want = [tuple(x.clone() for x in pipe.forward(h.to(gpu))) for h in host]
    torch.cuda.synchronize()
    busy = torch.empty(512 << 20, dtype=torch.uint8, device=gpu)
    outs, lag = [], pipe.voxelizer.LAG + 1
    for k in range(len(host) + lag):
        if k < len(host):
            for _ in range(4):
                busy.add_(1)                                    # the copy below queues behind ~1 ms of work
            c = host[k].to(gpu, non_blocking=True)
            r = pipe.forward_overlapped(c)
            del c                                               # the caller drops the cloud at once ...
            junk = torch.full((2, 15000, 4), float("nan"), device=gpu)   # ... and the same block size is asked for again
            del junk
        else:
            r = pipe.forward_overlapped(None)
        assert (r is None) == (k < lag)
        if r is not None:
            outs.append(tuple(x.clone() for x in r))
    torch.cuda.synchronize()
    assert len(outs) == len(host)
    for (c, r), (wc, wr) in zip(outs, want):
        assert torch.isfinite(c).all() and (c - wc).abs().max().item() <= 2e-6 and (r - wr).abs().max().item() <= 2e-6


def test_fused_forms_fall_back_to_the_dense_path_with_a_data_mean(gpu):
    """One behaviour for one condition: with a dataset mean both fused forms run the dense path --
    forward_fused like forward, forward_fused_pipelined like forward_pipelined (same lag)."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    cfg = VoxelConfig.square(16.0, 0.2, 3000, 16)
    mean = np.random.default_rng(0).normal(0, 0.1, 9 * 3000 * 16).astype(np.float32)
    pipe = PillarPipeline(cfg, feature_channels=16, device=gpu, seed=0, data_mean=mean)
    pipe.model.eval()
    clouds = [torch.from_numpy(synth.lidar_like(9000, 16.0, s)).to(gpu) for s in range(3)]
    want = [tuple(x.clone() for x in pipe.forward(c)) for c in clouds]
    got = [tuple(x.clone() for x in pipe.forward_fused(c)) for c in clouds]
    outs = []
    for c in clouds + [None] * pipe.voxelizer.LAG:
        r = pipe.forward_fused_pipelined(c)
        if r is not None:
            outs.append(tuple(x.clone() for x in r))
    assert len(outs) == 3
    for w, g, o in zip(want, got, outs):
        assert torch.equal(w[0], g[0]) and torch.equal(w[1], g[1]) and torch.equal(w[0], o[0]) and torch.equal(w[1], o[1])


def test_configs4_canvas_end_to_end(gpu, oracle):
    """BASELINE configs[4]'s sizes through the whole forward on the GPU (SURVEY section 7 hard part 8: at a 1000x1000 canvas
    the stride-4 up block needs output_padding 3, model/model.py:122-129): 200k-point sweep, P=30000, B=1.  forward ==
    the model on the oracle's pillars; the fused one-launch form agrees within 1e-4."""
    import torch
    from pp_amd import synth
    from pp_amd.pipeline import PillarPipeline
    from pp_amd.voxelizer import VoxelConfig
    from util import oracle_stage
    cfg = VoxelConfig.square(100.0, 0.2, 30000, 100)
    pipe = PillarPipeline(cfg, device=gpu, seed=0)
    pipe.model.eval()
    assert pipe.model.backbone.up3.conv2d_t.output_padding == (3, 3)
    pts = synth.lidar_like(200000, 100.0, 5)
    dpts = torch.from_numpy(pts).to(gpu)
    cl, rg = pipe.forward(dpts)
    assert cl.shape == (1, 18, 500, 500) and rg.shape == (1, 16, 500, 500)
    ref_p, ref_i, m = oracle_stage(oracle, pts, 30000, 100, 100.0, 0.2, order=cfg.order)
    assert m > 30000                                            # the overflow regime, as in the bench
    with torch.no_grad():
        cl2, rg2 = pipe.model(torch.from_numpy(ref_p)[None].to(gpu), torch.from_numpy(ref_i)[None].to(gpu))
    assert torch.equal(cl, cl2) and torch.equal(rg, rg2)
    cl, rg = cl.clone(), rg.clone()
    outs = []
    for c in [dpts, dpts] + [None] * pipe.voxelizer.LAG:
        r = pipe.forward_fused_pipelined(c)
        if r is not None:
            outs.append((r[0].clone(), r[1].clone()))
    assert len(outs) == 2
    for c, r in outs:
        assert (c - cl).abs().max().item() <= 1e-4 and (r - rg).abs().max().item() <= 1e-4
    # the dense pipelined form: bit-identical to forward
    outs = [pipe.forward_pipelined(c) for c in [dpts] + [None] * pipe.voxelizer.LAG]
    assert torch.equal(outs[-1][0], cl) and torch.equal(outs[-1][1], rg)
