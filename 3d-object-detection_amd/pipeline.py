"""Device-resident sample pipeline: raw points -> pillars -> network (-> loss).

Counterpart of what /root/reference does per step between the lidar file and
the loss: ``PPDataset.__getitem__``'s voxel stage and target stage
(data/dataset.py:88-120) on the HIP kernels, then ``PPModel`` / ``PPLoss``
(train.py:144-145, evaluate.py:228) on PyTorch-ROCm.  Nothing crosses PCIe
except the raw points (0.96 MB per 60k-point sweep) and the boxes.
"""
import functools

import numpy as np
import torch

from . import boxes
from .augment import Augmenter, Paster, draw, draw_paste, extend_gts
from .loss import FusedPPLoss, PPLoss
from .model import PPModel, check_inference_precision
from .targets import TargetAssigner
from .voxelizer import PillarVoxelizer, VoxelConfig


#: the backbone blocks whose stride-1 layers PillarPipeline switches to the split-fp16 kernel: those of down1, down2,
#: down3, up1 at whose headline shape (B = 4, 500 x 500 canvas) the slowest of three legs of 500 launches of
#: ``_conv_split`` was ahead of the fastest Winograd leg (profiles/r29/NOTES.md)
SPLIT_MMA_BLOCKS = ("down1", "down2", "down3", "up1")


class PillarPipeline:
    def __init__(self, vox_cfg: VoxelConfig, anchor_cfg: boxes.AnchorConfig = None,
                 feature_channels=64, num_classes=9, reg_dims=8, device=None, seed=0,
                 pos_thresh=0.6, with_targets=False, data_mean=None, precision="f32",
                 strided=False, augment=None, paste=None, fused_loss=False, split_mma=True, split_strided=False,
                 split_train=False, split_wgrad=False, split_train_s2=False, split_train_up=False):
        """``augment``: an ``augment.AugmentConfig`` -- ``train_forward_backward(..., augment_rng=rng)`` then augments
        the points and the boxes on the device before the voxelizer and the assigner (needs ``with_targets``).
        ``paste``: ``(augment.GtBank, augment.PasteConfig)`` -- ground-truth sampling before that augmentation, so
        pasted objects get the per-object noise and the global transform like native ones (needs ``augment``; for
        pasting alone pass ``AugmentConfig.identity()``).
        ``precision``: ``PPModel.set_inference_precision`` ("f32", "fp16" for fp16-operand MFMA in the
        backbone's stride-1 layers at inference, or "fp16-up" for those and the two strided transposed convolutions);
        ``strided``: its keyword of the same name (the down blocks' stride-2 convolutions too; not with "f32").
        ``split_mma``: with ``precision="f32"``, the stride-1 layers of ``SPLIT_MMA_BLOCKS`` run the split-fp16 MFMA
        kernel (``PPDownBlock.split_mma``, csrc/pp_conv_split.hip: f32-grade results on the fp16 matrix pipe) instead
        of the Winograd kernel; False keeps every block on Winograd, and so does ``with_targets`` (a training
        pipeline: activations beyond the kernel's window, |x| >= 65520, come out as NaN).
        ``split_strided``: with ``precision="f32"`` only, and not with ``with_targets`` (both a ``ValueError``): the
        stride-2 convolutions that open down1, down2 and down3 (``PPDownBlock.split_mma_s2``) and the transposed
        convolutions of up2 and up3 (``PPUpBlock.split_mma_up``) run split-fp16 MFMA kernels of their own
        (csrc/pp_conv_s2_split.hip, csrc/pp_convt_split.hip) instead of MIOpen's convolutions and an epilogue pass:
        with it the f32 backbone makes no MIOpen 3x3 call.  Independent of ``split_mma``; the same window.
        ``split_train``: with ``with_targets`` and ``precision="f32"`` only (else a ``ValueError``): in train() the
        stride-1 layers of down1, down2 and down3 (``PPDownBlock.split_train``) run their forward conv and their data
        gradient on the split-fp16 MFMA kernel and their ReLU -> BatchNorm tail channels-last
        (include/pp_conv_train.h) instead of MIOpen's NCHW f32 convolutions; the weight gradient stays MIOpen's.
        Window: forward activations with |x| >= 65520 give NaN.  A stride-1 layer's input is always a BatchNorm
        output, and the gradients are rescaled per tensor by a power of two and have no window.  The training tails
        keep that NaN through their ReLU (as ``torch.relu`` does), so the loss and the gradients of such a step are
        NaN and ``optim.FusedAdam(skip_nonfinite=True)`` drops it, with any of these switches.  A dropped step keeps
        every parameter, both moments and the running statistics of every layer whose batch statistics were not
        finite; it does not keep the running statistics of the layers before that one, which are updated as in any
        step, nor ``num_batches_tracked`` (incremented on the host without a wait).  eval() is untouched.
        ``split_wgrad``: with ``split_train`` only (else a ``ValueError``): those layers' weight gradient too
        (``PPDownBlock.split_wgrad``) runs on the split-fp16 MFMA pipe, a deterministic split-K kernel on the
        channels-last tensors as they lie (include/train/pp_conv_wgrad.h), with the data gradient's power-of-two scale
        of ``dz``: no MIOpen call is left in those 13 layers.  The same window as ``split_train``.
        ``split_train_s2``: with ``split_train`` only (else a ``ValueError``): the stride-2 conv that opens each of
        down1, down2 and down3 (``PPDownBlock.split_train_s2``) runs forward and data gradient on the split-fp16
        kernels too, channels-last with the channels-last tail (include/train/pp_conv_s2_train.h), and the blocks hand
        channels-last tensors on: no layout copy is left inside a down block.  Its weight gradient stays MIOpen's
        unless ``split_wgrad`` is on as well, which then covers these three layers too.  The same window.
        ``split_train_up``: with ``with_targets`` and ``precision="f32"`` only (else a ``ValueError``), independent of
        the down blocks' switches: in train() the transposed convs of up1, up2 and up3 (``PPUpBlock.split_train_up``) run
        on the split-fp16 MFMA kernels in all three directions, forward, data gradient and weight gradient, with the
        channels-last tail (include/train/pp_convt_train.h) instead of MIOpen's; there is no MIOpen weight-gradient
        variant for these blocks.  The same window: the up blocks' inputs are BatchNorm outputs.  eval() is untouched.
        ``fused_loss``: ``train_forward_backward`` computes the loss and its gradients with ``loss.FusedPPLoss`` (three
        HIP launches, no host wait) instead of ``PPLoss``."""
        check_inference_precision(precision, strided)      # before anything is built
        self.check_split_strided(split_strided, precision, with_targets)
        self.check_split_train(split_train, precision, with_targets)
        self.check_split_wgrad(split_wgrad, split_train)
        self.check_split_train_s2(split_train_s2, split_train)
        self.check_split_train_up(split_train_up, precision, with_targets)
        self.check_paste_argument(paste, augment)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.vox_cfg = vox_cfg
        h, w = vox_cfg.canvas_height, vox_cfg.canvas_width
        if anchor_cfg is None:
            anchor_cfg = boxes.AnchorConfig(fm_height=(h + 1) // 2, fm_width=(w + 1) // 2)
        self.anchor_cfg = anchor_cfg
        # data_mean: the optional pillar_means.pkl of train.py:61 / evaluate.py:207
        self.voxelizer = PillarVoxelizer(vox_cfg, device=self.device, data_mean=data_mean)
        torch.manual_seed(seed)  # model/model.py:9
        self.model = PPModel(9, feature_channels, anchor_cfg.per_cell * num_classes,
                             anchor_cfg.per_cell * reg_dims, h, w).to(self.device)
        self.model.set_inference_precision(precision, strided)
        # inference: the head reads the up blocks' outputs where they lie (PPDetectionHead.fused_parts)
        self.model.det_head.fused_parts = True
        # ... and the stride-1 layers of the blocks that measured ahead of the Winograd kernel run split-fp16.  Not in
        # a pipeline built for training: it evaluates weights between optimizer steps, whose activations nothing
        # bounds, and the kernel's window ends at |x| < 65520 (a step at lr 0.05 took down3's inputs to 7.9e4)
        for name in SPLIT_MMA_BLOCKS if split_mma and precision == "f32" and not with_targets else ():
            getattr(self.model.backbone, name).split_mma = True
        # ... and, on request, the strided layers on their split-fp16 kernels
        if split_strided:
            bb = self.model.backbone
            for blk in (bb.down1, bb.down2, bb.down3):
                blk.split_mma_s2 = True
            for blk in (bb.up2, bb.up3):
                blk.split_mma_up = True
        # ... and, on request, the training step's stride-1 convs (forward and data gradient) on the split-fp16 kernel
        if split_train:
            for blk in (self.model.backbone.down1, self.model.backbone.down2, self.model.backbone.down3):
                blk.split_train = True
                blk.split_wgrad = bool(split_wgrad)       # ... and their weight gradient
                blk.split_train_s2 = bool(split_train_s2)  # ... and the stride-2 conv that opens the block
        # ... and, on request, the up blocks' transposed convs in all three directions
        if split_train_up:
            for blk in (self.model.backbone.up1, self.model.backbone.up2, self.model.backbone.up3):
                blk.split_train_up = True
        self.loss = FusedPPLoss(return_p=False) if fused_loss else PPLoss()
        self.assigner = None
        if with_targets:
            # anchors evaluated on the fly in the target kernels (no per-anchor arrays)
            self.assigner = TargetAssigner(anchor_cfg, canvas_height=h,
                                           pos_thresh=pos_thresh, num_classes=num_classes,
                                           device=self.device)
        self.augmenter = None
        if augment is not None:
            if self.assigner is None:
                raise ValueError("augment needs with_targets=True: it feeds the target assigner")
            self.augmenter = Augmenter(vox_cfg, augment, device=self.device)
        self.paster = None
        if paste is not None:
            self.paster = Paster(vox_cfg, paste[0], paste[1], device=self.device)
        self._bufs = None
        self._fbufs = None
        self._cbuf = None
        self._cidx = None          # the indices of the last fused-scatter call: the canvas's non-zero pixels
        self._canvas_key = None
        #: forward_fused also fuses PPScatter and runs the backbone channels-last
        self.fused_scatter = True

    @staticmethod
    def check_split_strided(split_strided, precision, with_targets):
        """The constructor's check of ``split_strided``, before any device is touched."""
        if not split_strided:
            return
        if precision != "f32":
            raise ValueError(f"split_strided=True goes with precision \"f32\" only, not {precision!r}: the fp16 modes "
                             "have kernels of their own for these layers (\"fp16-up\", strided=True)")
        if with_targets:
            # an explicit request, unlike the default split_mma, which a training pipeline quietly leaves off
            raise ValueError("split_strided=True is for inference pipelines: nothing bounds a training pipeline's "
                             "activations between optimizer steps, and the kernels' window ends at |x| < 65520")

    @staticmethod
    def check_split_train(split_train, precision, with_targets):
        """The constructor's check of ``split_train``, before any device is touched."""
        if not split_train:
            return
        if not with_targets:
            raise ValueError("split_train=True needs with_targets=True: it switches the training step's convolutions")
        if precision != "f32":
            raise ValueError(f"split_train=True goes with precision \"f32\" only, not {precision!r}: the fp16 modes "
                             "change the inference path of the same blocks")

    @staticmethod
    def check_split_wgrad(split_wgrad, split_train):
        """The constructor's check of ``split_wgrad``, before any device is touched."""
        if split_wgrad and not split_train:
            raise ValueError("split_wgrad=True needs split_train=True: it is the weight gradient of the layers that "
                             "split_train moves to the split-fp16 kernels")

    @staticmethod
    def check_split_train_up(split_train_up, precision, with_targets):
        """The constructor's check of ``split_train_up``, before any device is touched."""
        if not split_train_up:
            return
        if not with_targets:
            raise ValueError("split_train_up=True needs with_targets=True: it switches the training step's transposed "
                             "convolutions")
        if precision != "f32":
            raise ValueError(f"split_train_up=True goes with precision \"f32\" only, not {precision!r}: the fp16 modes "
                             "are inference modes")

    @staticmethod
    def check_split_train_s2(split_train_s2, split_train):
        """The constructor's check of ``split_train_s2``, before any device is touched."""
        if split_train_s2 and not split_train:
            raise ValueError("split_train_s2=True needs split_train=True: it is the first layer of the blocks that "
                             "split_train moves to the split-fp16 kernels")

    @staticmethod
    def check_paste_argument(paste, augment):
        """The constructor's check of ``paste``, before any device is touched."""
        if paste is None:
            return
        if augment is None:
            raise ValueError("paste needs augment: the pasted boxes go through the augmenter "
                             "(for pasting alone pass AugmentConfig.identity())")
        if not isinstance(paste, (tuple, list)) or len(paste) != 2:
            raise ValueError("paste: a (GtBank, PasteConfig) pair")
        paste[1].validate()

    def _buffers(self, batch):
        cfg = self.vox_cfg
        if self._bufs is None or self._bufs[0].shape[0] != batch:
            self._bufs = (torch.empty((batch, 9, cfg.max_pillars, cfg.max_points_per_pillar),
                                      dtype=torch.float32, device=self.device),
                          torch.empty((batch, cfg.max_pillars, 3), dtype=torch.int64, device=self.device))
        return self._bufs

    def voxelize(self, points, n_points=None):
        if points.dim() == 2:
            points = points.unsqueeze(0)
        return self.voxelizer(points, n_points=n_points, out=self._buffers(points.shape[0]))

    @torch.no_grad()
    def forward(self, points, n_points=None):
        """evaluate.py:216-228: voxel stage + network forward (inference)."""
        pillars, indices = self.voxelize(points, n_points)
        return self.model(pillars, indices)

    @torch.no_grad()
    def forward_pipelined(self, points, n_points=None):
        """The same forward as a software pipeline over consecutive batches (what the reference's
        DataLoader prefetch amounts to, train.py:120-121): the voxelizer's ONE launch per call runs the
        split stage of ``points``, the tile and order stages of the two previous calls' batches and the emit
        stage of the batch before those (``PillarVoxelizer.submit``), and the network runs on that oldest
        batch.  Returns its ``(cls, reg)`` -- or ``None`` for the first ``PillarVoxelizer.LAG`` calls.  ``points=None`` drains."""
        B = self.voxelizer._inflight[-1] if getattr(self.voxelizer, "_inflight", None) else None
        r = self.voxelizer.submit(points, n_points=n_points, out=self._buffers(B) if B else None)
        return None if r is None else self.model(r[0], r[1])

    @torch.no_grad()
    def forward_overlapped(self, points, n_points=None):
        """``forward_pipelined`` with the voxelizer's launch on a SECOND stream, side by side with the network (what
        the reference's DataLoader workers do on CPU cores, train.py:120-121): call i launches ``k_step`` on the side
        stream (it emits an older batch into one of two output buffers) and, on the caller's stream, runs the network
        on the batch the PREVIOUS call's launch emitted into the other buffer.  The two only meet through events that
        were recorded a whole step earlier, so neither queue waits: the voxelizer leaves the step's critical path.
        ``points`` (and ``n_points`` if it is a tensor) may be produced on the caller's stream right before the call
        -- a ``non_blocking`` copy, an ingest kernel -- and dropped right after it: the side stream waits for an event
        recorded on the caller's stream AT ENTRY (between two calls that stream holds only the previous network pass
        and whatever produced ``points``, so the wait also covers "buffer k was read by the previous call's network"
        and costs the overlap nothing), and the tensors are ``record_stream``-ed on the side stream, so the caching
        allocator does not hand their memory to a main-stream allocation while the side-stream launch still reads it.
        Returns ``(cls, reg)`` of the batch handed in ``PillarVoxelizer.LAG + 1`` calls ago, else ``None``;
        ``points=None`` drains."""
        ov = getattr(self, "_ov", None)
        if ov is None:
            ov = self._ov = {"stream": torch.cuda.Stream(device=self.device), "i": 0, "bufs": [None, None],
                             "vox_done": [torch.cuda.Event(), torch.cuda.Event()], "entry": torch.cuda.Event(),
                             "ready": [None, None]}
        main = torch.cuda.current_stream(self.device)
        i, side = ov["i"], ov["stream"]
        k = i % 2
        # everything the caller's stream holds now -- the producer of `points`, the previous call's network pass that
        # read buffer k -- is ordered before the side stream's launch
        ov["entry"].record(main)
        side.wait_event(ov["entry"])
        for t_ in (points, n_points):
            if torch.is_tensor(t_) and t_.is_cuda:
                t_.record_stream(side)
        B = self.voxelizer._inflight[-1] if getattr(self.voxelizer, "_inflight", None) else None
        with torch.cuda.stream(side):
            if B and (ov["bufs"][k] is None or ov["bufs"][k][0].shape[0] != B):
                cfg = self.vox_cfg
                ov["bufs"][k] = (torch.empty((B, 9, cfg.max_pillars, cfg.max_points_per_pillar), dtype=torch.float32,
                                             device=self.device),
                                 torch.empty((B, cfg.max_pillars, 3), dtype=torch.int64, device=self.device))
            r = self.voxelizer.submit(points, n_points=n_points, out=ov["bufs"][k] if B else None)
            ov["vox_done"][k].record(side)
        ov["ready"][k] = r
        ov["i"] = i + 1
        prev = ov["ready"][1 - k]
        ov["ready"][1 - k] = None
        out = None
        if prev is not None:
            main.wait_event(ov["vox_done"][1 - k])
            out = self.model(prev[0], prev[1])
        return out

    @torch.no_grad()
    def forward_fused(self, points, n_points=None):
        """Inference with PPFeatureNet fused into the voxelizer:
        the dense [9,P,N] tensor and the [64,P,N] intermediate never exist.  Needs
        ``model.eval()`` (BatchNorm as an affine map)."""
        if self.model.training:
            raise RuntimeError("forward_fused is inference only: call model.eval() first")
        if self.voxelizer.data_mean is not None:
            # a data mean makes the zero-padded slots non-zero: nothing to skip, use the dense path
            return self.forward(points, n_points)
        pfn_params = self.model.feature_net.fused_table(self.device)   # tracks the weights' versions
        if points.dim() == 2:
            points = points.unsqueeze(0)
        B = points.shape[0]
        P = self.vox_cfg.max_pillars
        if self._fbufs is None or self._fbufs[0].shape[0] != B:
            self._fbufs = (torch.empty((B, 64, P), dtype=torch.float32, device=self.device),
                           torch.empty((B, P, 3), dtype=torch.int64, device=self.device))
        if self.fused_scatter:
            # ... and PPScatter too: the emit kernel writes each pillar's 64 features to its
            # channels-last canvas pixel
            H, W = self.model.scatter.h, self.model.scatter.w
            cbuf = self._canvas(B, H, W)
            # The canvas and ITS index buffer are written by this branch only (the feature path below has its
            # own indices): after the first call only the previous call's pixels are non-zero, and only those
            # are cleared again.  The key is dropped before the call, so an error cannot leave a stale one.
            if self._cidx is None or self._cidx.shape[0] != B:
                self._cidx = torch.empty((B, P, 3), dtype=torch.int64, device=self.device)
                self._canvas_key = None
            key = (cbuf.data_ptr(), self._cidx.data_ptr(), B)
            reuse = self._canvas_key == key
            self._canvas_key = None
            canvas, _ = self.voxelizer.pfn_canvas(points, pfn_params, (H, W), n_points=n_points,
                                                  out=(cbuf, self._cidx), reuse=reuse)
            self._canvas_key = key
            return self.model.forward_canvas(canvas)
        feats, indices = self.voxelizer.pfn(points, pfn_params, n_points=n_points, out=self._fbufs)
        return self.model.forward_features(feats, indices)

    @torch.no_grad()
    def forward_fused_pipelined(self, points, n_points=None):
        """``forward_fused`` as a software pipeline over consecutive batches: ONE voxelizer launch per call
        (``PillarVoxelizer.submit_pfn_canvas``: the split stage of ``points``, the tile and order stages of the two
        previous batches, and the emit stage of the batch before those AS the fused feature net writing straight
        into the channels-last canvas), and the network runs on that oldest batch's canvas.  Returns its
        ``(cls, reg)`` -- ``None`` for the first ``PillarVoxelizer.LAG`` calls; ``points=None`` drains."""
        if self.model.training:
            raise RuntimeError("forward_fused_pipelined is inference only: call model.eval() first")
        if self.voxelizer.data_mean is not None:
            # as forward_fused: a data mean makes the zero-padded slots non-zero, nothing to skip -- the dense
            # pipelined path (same pipeline, same lag: the batches in flight are shared between the two forms)
            return self.forward_pipelined(points, n_points)
        pfn_params = self.model.feature_net.fused_table(self.device)
        H, W = self.model.scatter.h, self.model.scatter.w
        r = self.voxelizer.submit_pfn_canvas(points, pfn_params, (H, W), n_points=n_points, channels_last=True)
        return None if r is None else self.model.forward_canvas(r[0])

    def _canvas(self, B, H, W):
        if self._cbuf is None or self._cbuf.shape != (B, 64, H, W):
            self._cbuf = torch.empty((B, 64, H, W), dtype=torch.float32, device=self.device,
                                     memory_format=torch.channels_last)
        return self._cbuf

    def upload_ground_truth(self, g):
        """Host box arrays (centers / wlh / yaw / classes, canvas space) -> the device tuple
        ``TargetAssigner.assign_device`` consumes (image-space corners are derived here,
        utils/box_utils.py:19-32)."""
        return self.assigner._gt_to_device(g["centers"], g["wlh"], g["yaw"], g["classes"])

    def upload_ground_truth_batch(self, gts):
        """The boxes of ALL samples of a step in one device buffer (one host-to-device copy):
        ``(g_counts, packed)``, what ``TargetAssigner.assign_batch_device`` and
        ``train_forward_backward`` consume."""
        return self.assigner.upload_batch(gts)

    def train_forward_backward(self, points, gts, n_points=None, shard_ctx=None, augment_rng=None):
        """train.py:139-147 without the optimizer: voxel stage, target stage, forward,
        loss, backward.  ``gts`` is a list (one per sweep) of dicts with
        centers / wlh / yaw / classes in canvas space.  With a multi-rank ``shard_ctx`` the
        back-propagated loss is ``shard.global_batch_loss`` (this rank's share of the ONE loss
        the reference computes over the gathered batch); the returned scalars stay the local
        PPLoss values.  With an ``augment`` config at construction, a ``numpy.random.Generator`` as ``augment_rng``
        and ``gts`` as a list of dicts, the step trains on an augmented copy of the points and the boxes
        (``augment.Augmenter``: the draws on the host, one upload, two launches); with ``paste`` too, bank objects
        are pasted first (``augment.Paster``); every other call is untouched."""
        if (self.augmenter is not None and augment_rng is not None and not isinstance(gts, tuple)
                and all(isinstance(g, dict) for g in gts)):
            if points.dim() == 2:
                points = points.unsqueeze(0)
            if self.paster is not None:
                ids = draw_paste(self.paster.cfg, augment_rng, self.paster.bank, gts)
                gts, c_counts = extend_gts(self.paster.bank, gts, ids)
            counts = [int(np.asarray(g["yaw"]).reshape(-1).shape[0]) for g in gts]
            g_counts, packed = self.augmenter.upload_batch(gts, draw(self.augmenter.cfg, augment_rng, counts))
            points = points.contiguous()
            if self.paster is not None:
                points, n_points, _ = self.paster.apply(points, n_points, (g_counts, packed), c_counts, ids)
            # the pasted cloud is this step's own buffer: augment it in place
            points, gts, _, _ = self.augmenter.apply(points, n_points, g_counts, packed,
                                                     out=points if self.paster is not None else None)
        pillars, indices = self.voxelize(points, n_points)
        if isinstance(gts, tuple) and len(gts) == 2 and torch.is_tensor(gts[1]):
            cls_t, reg_t = self.assigner.assign_batch_device(*gts)
        elif all(isinstance(g, dict) for g in gts):
            cls_t, reg_t = self.assigner.assign_batch(gts)
        else:
            # per-sample device tuples of upload_ground_truth(): one launch per sample
            targets = [self.assigner.assign_device(*g) if isinstance(g, tuple)
                       else self.assigner.assign(g["centers"], g["wlh"], g["yaw"], g["classes"]) for g in gts]
            cls_t = torch.stack([t[0] for t in targets])
            reg_t = torch.stack([t[1] for t in targets])
        cls, reg = self.model(pillars, indices)
        p, cls_loss, reg_loss, ort_loss, total = self.loss(cls, reg, cls_t, reg_t)
        if shard_ctx is not None and shard_ctx.distributed:
            from . import shard
            n_pos = (reg_t[..., 0] == 1).sum()
            shard.global_batch_loss(shard_ctx, self.loss, cls_loss, reg_loss, ort_loss, n_pos).backward()
        else:
            total.backward()
        return cls_loss.detach(), reg_loss.detach(), ort_loss.detach(), total.detach()

    def train_step(self, points, gts, optimizer, n_points=None, shard_ctx=None, augment_rng=None):
        """train.py:139-148 whole: ``optimizer.zero_grad(set_to_none=True)``, ``train_forward_backward`` and the
        optimizer step; returns the four losses.  With an ``optim.FusedAdam`` and a distributed ``shard_ctx`` the
        step packs the gradients into the optimizer's flat buffer, all-reduces that once (``shard.allreduce_flat``)
        and updates from it; with any other optimizer it is ``shard.allreduce_gradients`` and ``optimizer.step()``."""
        from . import shard
        from .optim import FusedAdam
        optimizer.zero_grad(set_to_none=True)
        losses = self.train_forward_backward(points, gts, n_points=n_points, shard_ctx=shard_ctx,
                                             augment_rng=augment_rng)
        distributed = shard_ctx is not None and shard_ctx.distributed
        if isinstance(optimizer, FusedAdam):
            optimizer.step(grad_reduce=functools.partial(shard.allreduce_flat, shard_ctx) if distributed else None)
        else:
            if distributed:
                shard.allreduce_gradients(shard_ctx, self.model.parameters())
            optimizer.step()
        return losses
