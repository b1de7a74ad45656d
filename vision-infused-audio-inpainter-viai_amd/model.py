"""AudioModel — the G+D train step of the inpainting GAN on the HIP kernels.

The reference's `Models/Whole_Sync_inpainting_modify.AudioModel` is ABSENT from
the snapshot; its interface is pinned only by the call sites in
train_whole_sync.py:49-112,159-183 and utils/util.py:146-173.  This class
implements that interface; the step itself follows the pix2pix ordering the
reference credits (README.md:39) and is the build's declared spec:

    s_in  = s * mask
    fake  = Mel_Decoder(Mel_Encoder(s_in), s.size())
    D:  loss_D = 0.5*[GAN(netD(fake.detach()), False) + GAN(netD(s), True)] -> Adam(D)
    G:  loss_G = GAN(netD(fake), True) + lambda_L1 * L1(fake, s)            -> Adam(E, G)

Memory layout: all parameters of an optimizer live in ONE flat fp32 arena (and
their gradients / Adam moments in three more), so the optimizer is a single
streaming kernel and data-parallel gradient exchange is one RCCL all-reduce per
optimizer with no packing copies (exchange.GradExchange).  The whole step can
be captured into HIP graphs (three segments, split at the two all-reduce
points: step_capture.CapturedStep).
"""
from __future__ import annotations

import contextlib
import math
import os
import weakref
from collections import OrderedDict

import torch
import torch.nn as nn

from . import ops
from ._lib import check, load as lib
from .exchange import GradExchange, plan_buckets
from .networks import (ImageEmbedding2, MelDecoder, MelDecoderImage, MelDiscriminator, MelEncoder, MultiScaleDiscriminator,
                       to_nchw_view)
from .step_capture import CapturedStep


class StepConfig:
    lr = 2e-4
    beta1 = 0.5
    beta2 = 0.999
    eps = 1e-8
    lambda_l1 = 100.0
    use_lsgan = False
    batch_size = 16
    cin_channels = 256          # mel bins F
    max_mel_lengths = 256       # frames T
    name = "viai"
    save_optimizer_state = True
    # BASELINE configs[2] / configs[3] (declared adaptations):
    use_video = False           # ResNet-18 ImageEmbedding2 fused into the G bottleneck through MelDecoderImage; when the
                                # bottleneck height h > 1 (F = 256) the video feature is TILED over h
    num_D = 1                   # > 1: multi-scale D = num_D MelDiscriminators on an avg-pool pyramid
    lambda_contrast = 0.0       # weight of L2ContrastiveLoss(audio bottleneck, video feature)  (`EmbeddingL2_item`)
    contrast_margin = 1.0


class FlatArena:
    """Moves the parameters of `modules` into one contiguous fp32 buffer (views
    keep every nn.Parameter usable as before) and gives them gradient views of a
    second buffer, so `.grad` accumulation lands in the arena."""

    ALIGN = 64

    def __init__(self, named_params):
        self.names, self.params, self.offsets = [], [], []
        off = 0
        for name, p in named_params:
            self.names.append(name)
            self.params.append(p)
            self.offsets.append(off)
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.size = off
        dev = self.params[0].device
        self.flat = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)

    def zero_grad(self):
        self.grad.zero_()
        for p, o in zip(self.params, self.offsets):      # re-attach in case something replaced .grad
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad[o:o + p.numel()].view(p.shape)


class FusedAdam:
    """torch.optim.Adam semantics (no amsgrad / weight decay) as one HIP kernel over a FlatArena.
    The step counter and bias corrections live on the device (graph-replayable)."""

    def __init__(self, arena: FlatArena, lr, betas, eps, stateless=()):
        """`stateless`: indices of parameters the forward never reaches (e.g. MelDecoder.convblock1.*): torch.optim.Adam keeps
        no state for a parameter whose .grad stays None, and neither does state_dict() here (their gradient is exactly zero, so
        the kernel leaves them and their moments untouched anyway)."""
        self.arena = arena
        self.stateless = frozenset(int(i) for i in stateless)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(arena.flat)
        self.exp_avg_sq = torch.zeros_like(arena.flat)
        self.state = torch.tensor([0.0, self.lr, 1.0, 1.0], dtype=torch.float64, device=arena.flat.device)

    def zero_grad(self):
        self.arena.zero_grad()

    def set_lr(self, lr):
        """writes the device-side rate on the CURRENT stream: callers that run the optimizer on another stream (AudioModel's deferred
        G update) order the write themselves -- use AudioModel.set_lr"""
        self.lr = float(lr)
        self.state[1] = self.lr

    def step(self, grad_scale=1.0):
        ops.adam_step(self.arena.flat, self.arena.grad, self.exp_avg, self.exp_avg_sq, self.state,
                      self.betas[0], self.betas[1], self.eps, grad_scale)
        ops.weights_changed(self.arena.params, owner=self)     # the kernel wrote the arena: re-pack every conv weight image in one launch

    # torch.optim.Adam-compatible (de)serialisation so utils/util.py:149-150 style checkpoints interchange
    def state_dict(self):
        step = float(self.state[0].item())
        st = {}
        if step > 0:                                      # torch creates the per-parameter state lazily, at the first step
            for i, (p, o) in enumerate(zip(self.arena.params, self.arena.offsets)):
                if i in self.stateless:
                    continue
                n = p.numel()
                st[i] = {"step": torch.tensor(step), "exp_avg": self.exp_avg[o:o + n].view(p.shape).detach().cpu().clone(),
                         "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).detach().cpu().clone()}
        # the param_group of the installed torch.optim.Adam (its key set differs between torch versions), with our values
        group = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()["param_groups"][0]
        group["params"] = list(range(len(self.arena.params)))
        return {"state": st, "param_groups": [group]}

    def load_state_dict(self, sd):
        step = 0.0
        for i, (p, o) in enumerate(zip(self.arena.params, self.arena.offsets)):
            s = sd["state"].get(i)
            if s is None:
                continue
            n = p.numel()
            self.exp_avg[o:o + n].copy_(s["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(s["exp_avg_sq"].reshape(-1))
            step = max(step, float(s["step"]))
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(g["lr"]), tuple(g["betas"]), float(g["eps"])
        self.state.copy_(torch.tensor([step, self.lr, self.betas[0] ** step, self.betas[1] ** step], dtype=torch.float64))


def make_time_mask(batch, frames, blank_length, generator=None, device="cpu"):
    """One full-height time gap [t0, t0+L) per clip (misc/pipeline2.png); t0 ~ U{T/8 .. 5T/8}."""
    lo, hi = frames // 8, (5 * frames) // 8
    t0 = torch.randint(lo, hi + 1, (batch,), generator=generator)
    t0 = torch.clamp(t0, max=frames - blank_length)
    ar = torch.arange(frames)[None, :]
    m = ((ar < t0[:, None]) | (ar >= t0[:, None] + blank_length)).float()
    return m.view(batch, 1, 1, frames).to(device)


class AudioModel:
    """Interface inferred from train_whole_sync.py:49,50,68,75-85,91-112,145,159-183."""

    def __init__(self, hparams=None, device=None, process_group=None, use_graph=False, use_plan=False):
        self.hparams = hparams if hparams is not None else StepConfig()
        hp = self.hparams
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise RuntimeError("AudioModel runs on an MI355X (HIP kernels); there is no CPU path")
        self.use_video = bool(getattr(hp, "use_video", False))
        self.num_D = int(getattr(hp, "num_D", 1))
        self.Mel_Encoder = MelEncoder(hp).to(self.device)
        self.Mel_Decoder = (MelDecoderImage(hp) if self.use_video else MelDecoder(hp)).to(self.device)
        self.netD = (MultiScaleDiscriminator(self.num_D) if self.num_D > 1 else MelDiscriminator()).to(self.device)
        self.VideoEncoder = ImageEmbedding2(hp).to(self.device) if self.use_video else None
        self.video = self.flow = None
        self.cfg = StepConfig()
        for k in ("lr", "beta1", "beta2", "eps", "lambda_l1", "use_lsgan", "lambda_contrast", "contrast_margin"):
            if hasattr(hp, k):
                setattr(self.cfg, k, getattr(hp, k))
        self._build_optimizers()
        self.pg = process_group
        self.world = 1
        self._force_allreduce = False      # tests: run the RCCL exchange even at world size 1 (identity)
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
        self.train = 1
        self.update_wavenet = False
        self.blank_length = max(getattr(hp, "max_mel_lengths", 256) // 4, 1)
        self.current_lr = self.cfg.lr
        self.reconstruct_loss_item = 0.0
        self.EmbeddingL2_item = 0.0
        self.loss_mel_L1_item = 0.0
        self.mel_net_norm = None
        self.video_net_norm = None
        self.losses = torch.zeros(6, device=self.device)      # loss_D, loss_G, loss_G_GAN, loss_L1, loss_D_real, EmbeddingL2
        self.mel = self.mask = self.fake = None
        self._wmax = None
        # use_plan: the step is stream-captured once and replayed from C as a launch plan (csrc/plan.hip): the eager step's
        # kernels, arguments, streams and cross-stream edges without the per-launch host work.  Shares the segment structure
        # (and the static-buffer discipline) of graph mode, so it sets use_graph too.
        self.use_plan = bool(use_plan)
        self.use_graph = bool(use_graph) or self.use_plan
        self._captured = CapturedStep(self.device, self.use_plan)
        self._consts = {}
        # weight gradients trail on a side stream (ops.WGRAD_STREAM) in eager mode: -3.5 % step time on one MI355X.  Inside
        # a captured hipGraph the fork/join edges cost more than the overlap returns (+2 %), so graph mode stays on one
        # stream.  VIAI_WGRAD_STREAM=0/1 overrides.
        # With the visual branch the two ResNets already run as two chains on two streams (networks.ImageEmbedding2), each carrying its
        # own weight gradients; funnelling all of them through one trailing stream costs more than it overlaps (120.8 vs 124.1 ms).
        one_stream = self.use_graph and not self.use_plan
        from . import networks as _nets
        # (eager mode only: inside a capture ImageEmbedding2 does not fork its flow stream, so plan / graph mode keeps the trailing stream)
        two_chains = self.use_video and _nets.FLOW_STREAM and not self.use_graph
        side = os.environ.get("VIAI_WGRAD_STREAM", "0" if (one_stream or two_chains) else "1") != "0"
        self._wgrad_stream = torch.cuda.Stream(device=self.device) if side else None
        dreal = os.environ.get("VIAI_DREAL_STREAM", "0" if one_stream else "1") != "0"
        self._dreal_stream = torch.cuda.Stream(device=self.device) if dreal else None
        self._skip_exchange = False        # bench.py: measure the step without the collectives (comm_ms_exposed)

        def has_instance_norm(*mods):
            return any(isinstance(m, nn.InstanceNorm2d) for mod in mods if mod is not None for m in mod.modules())
        plan = plan_buckets(self.arena_G, self.arena_D, self.num_D, self.use_video,
                            has_instance_norm(self.Mel_Encoder, self.Mel_Decoder, self.VideoEncoder), has_instance_norm(self.netD))
        # (a weak reference: the exchange reads this model's two switches at every call, and must not keep the model alive)
        self.exchange = GradExchange(plan, weakref.proxy(self), self.pg, self.world, overlap=not self.use_graph, device=self.device)
        # what one segment of the step hands to the next
        self._fake = self._lc = self._loss_real = self._loss_fake = None
        self._g_exchanged = False                  # the G gradients of this step went through the exchange stream
        self._scalars_src = self._pred_fake_g = None
        self._stepped_since_range_check = False    # a train step ran since get_loss_items last looked at the weight range

    # ------------------------------------------------------------------ setup
    def _build_optimizers(self):
        c = self.cfg
        g_named = [("E." + n, p) for n, p in self.Mel_Encoder.named_parameters()] + \
                  [("G." + n, p) for n, p in self.Mel_Decoder.named_parameters()]
        if self.VideoEncoder is not None:
            g_named += [("V." + n, p) for n, p in self.VideoEncoder.named_parameters()]
        d_named = [("D." + n, p) for n, p in self.netD.named_parameters()]
        self.arena_G = FlatArena(g_named)
        self.arena_D = FlatArena(d_named)
        dead = tuple("G." + p for p in getattr(self.Mel_Decoder, "UNUSED_PREFIXES", ())) + \
            tuple("V." + p for p in getattr(self.VideoEncoder, "UNUSED_PREFIXES", ()))
        stateless = [i for i, n in enumerate(self.arena_G.names) if n.startswith(dead)] if dead else []
        self.optimizer_G = FusedAdam(self.arena_G, c.lr, (c.beta1, c.beta2), c.eps, stateless)
        self.optimizer_D = FusedAdam(self.arena_D, c.lr, (c.beta1, c.beta2), c.eps)

    # the gradient exchange (exchange.GradExchange), under the names tests and tools read
    _early_G = property(lambda self: self.exchange.plan.early_G)
    _late_G = property(lambda self: self.exchange.plan.late_G)
    _g_update_pending = property(lambda self: self.exchange.g_update_pending)

    def _exchanging(self):
        return self.exchange.exchanging()

    def _overlapped(self):
        return self.exchange.overlapped()

    def sync_pending_update(self):
        """the main stream waits for the deferred G exchange + Adam(E,G) + re-pack of the previous step (GradExchange.sync_pending_update)"""
        self.exchange.sync_pending_update()

    def load_states(self, E=None, G=None, D=None, V=None):
        """load state_dicts (e.g. the oracle's closed-form tables) without breaking the arenas."""
        if V is not None and self.VideoEncoder is None:
            raise ValueError("a VideoEncoder state was given but the model was built without use_video")
        self.sync_pending_update()
        for mod, sd in ((self.Mel_Encoder, E), (self.Mel_Decoder, G), (self.netD, D), (self.VideoEncoder, V)):
            if sd is None:
                continue
            own = mod.state_dict()
            for k, v in sd.items():
                own[k].copy_(v.to(own[k].device))
        self.weights_changed()

    def weights_changed(self):
        self.sync_pending_update()
        self._weights_changed()

    def set_lr(self, lr, which=("G", "D")):
        """learning rate of one or both optimizers (viai_amd.lrschedule.apply goes through here when handed the model).  The rate lives
        in the device-side Adam state; the deferred Adam(E,G) of the previous step may still be reading it on the exchange stream,
        so the write is ordered behind it."""
        self.sync_pending_update()
        if "G" in which:
            self.optimizer_G.set_lr(lr)
        if "D" in which:
            self.optimizer_D.set_lr(lr)
        self.current_lr = float(lr)
        return self.current_lr

    def _weights_changed(self):
        """Parameters were written outside the optimizers (checkpoint load, manual surgery): re-pack the conv weight
        images now.  Eager steps would notice through the tensor versions; a captured graph contains no per-layer pack
        launches (the optimizers' batched re-pack is what it replays), so it relies on this call."""
        ops.weights_changed(self.arena_G.params, owner=self.optimizer_G)
        ops.weights_changed(self.arena_D.params, owner=self.optimizer_D)

    # ------------------------------------------------------------- step pieces
    def get_blank_space_length(self, global_step):
        """mask-length curriculum hook (train_whole_sync.py:49); the policy is unpinned -> fixed T/4."""
        T = self.mel.shape[-1] if self.mel is not None else getattr(self.hparams, "max_mel_lengths", 256)
        self.blank_length = max(T // 4, 1)
        return self.blank_length

    def set_inputs(self, data, mask=None, video=None, flow=None):
        """data: the loader's 8-tuple (audio_loader.py:532: video, flow, c (B,C,T), x, y, g, lengths, paths) or a mel
        tensor (B,F,T)/(B,1,F,T) in [0,1].  Copies into static device buffers (graph-replay safe)."""
        if isinstance(data, (tuple, list)):
            video = data[0] if video is None else video
            flow = data[1] if flow is None else flow
        if self.use_video:
            if video is None or flow is None:
                raise ValueError("use_video: set_inputs needs the video (B,N,3,224,224) and flow (B,N,2,224,224) blocks")
            video = video.to(self.device, dtype=torch.float32)
            flow = flow.to(self.device, dtype=torch.float32)
            if self.video is None or self.video.shape != video.shape:
                self.video, self.flow = torch.empty_like(video), torch.empty_like(flow)
                self._captured.drop()           # new input shape: the captured graphs are stale
            self.video.copy_(video)
            self.flow.copy_(flow)
        mel = data[2] if isinstance(data, (tuple, list)) else data
        if mel.dim() == 3:
            mel = mel.unsqueeze(1)
        mel = mel.to(self.device, dtype=torch.float32, non_blocking=True)
        B, _, F, T = mel.shape
        if mask is None:
            mask = make_time_mask(B, T, min(self.blank_length, T), device=self.device)
        mask = mask.to(self.device, dtype=torch.float32).reshape(B, 1, 1, T)
        if self.mel is None or self.mel.shape != mel.shape:
            self.mel = torch.empty_like(mel)
            self.mask = torch.empty_like(mask)
            self._captured.drop()               # new input shape: the captured graphs are stale
        self.mel.copy_(mel)
        self.mask.copy_(mask)

    _captured = None        # __del__ of a half-built object: __init__ may have raised early

    def close(self):
        """release what the launch plans hold (CapturedStep.close); also runs from __del__"""
        if self._captured is not None:
            self._captured.close()

    def __del__(self):
        self.close()

    def plan_info(self):
        """per captured segment: nodes, kernels, kernels with a noted stream, copies, fills, streams, events, waits"""
        return self._captured.plan_info()

    def _gan(self, pred, real):
        t = 1.0 if real else 0.0
        if isinstance(pred, (list, tuple)):                  # multi-scale D: mean of the per-scale losses
            tot = None
            for p in pred:
                l = ops.mse_mean(p, t) if self.cfg.use_lsgan else ops.bce_mean(p, t)
                tot = l if tot is None else tot + l
            return tot / float(len(pred))
        return ops.mse_mean(pred, t) if self.cfg.use_lsgan else ops.bce_mean(pred, t)

    def _generate(self, s_nhwc, want_feats=False):
        """E (+ E_v) + G forward on NHWC; returns fake (B,F,T,1) and the contrastive term (or None)
        [+ the encoder maps and the video feature (B,256,1,T/16) when `want_feats`]."""
        B, F, T, _ = s_nhwc.shape
        feats = self.Mel_Encoder.forward_nhwc(s_nhwc.view(B, F, T), mask=self.mask)       # s_in = s * mask, where E.conv1 loads s
        if not self.use_video:
            fake = self.Mel_Decoder.forward_nhwc(feats, (F, T))
            return (fake, None, feats, None) if want_feats else (fake, None)
        f_v, _fea = self.VideoEncoder(self.video, self.flow)                 # (B,256,1,N/4), (B,512,N)
        h, w = feats[-1].shape[1], feats[-1].shape[2]
        if f_v.shape[3] != w:
            raise ValueError("use_video: need N = T/4 frames per clip (video steps %d != bottleneck steps %d)" % (f_v.shape[3], w))
        fv_nhwc = f_v.permute(0, 2, 3, 1)                                     # (B,1,w,256)
        head = self.Mel_Decoder._head_av(feats, fv_nhwc.expand(B, h, w, 256).permute(0, 3, 1, 2))   # tiled over h (declared adaptation)
        fake = self.Mel_Decoder.forward_nhwc(feats, (F, T), head=head)
        lc = None
        if self.cfg.lambda_contrast > 0:
            f_a = feats[-1].mean(dim=1).reshape(B * w, 256)
            lc = ops.l2_contrastive(f_a.contiguous(), fv_nhwc.reshape(B * w, 256).contiguous(), self.cfg.contrast_margin, False)
        return (fake, lc, feats, f_v) if want_feats else (fake, lc)

    def _const(self, v):
        """device scalar with a fixed value (gradient seeds), made once"""
        v = float(v)
        t = self._consts.get(v)
        if t is None:
            t = self._consts[v] = torch.full((), v, device=self.device, dtype=torch.float32)
        return t

    def _put(self, i, value):
        """losses[i] = value through an elementwise kernel: a `copy_` is a device-to-device memcpy, whose node parameters a
        stream capture does not give back (plan mode reads the captured launches)."""
        torch.mul(value.detach().reshape(1), 1.0, out=self.losses[i:i + 1])

    def _seg_forward_dstep(self):
        s = self.mel
        B, _, F, T = s.shape
        s_nhwc = s.view(B, F, T, 1)
        ops.begin_step(self.device)                    # re-arm the abs-max slots of the f16x2 backward kernels (one fill)
        self.optimizer_D.zero_grad()
        self.netD.requires_grad_(True)
        main = torch.cuda.current_stream()
        side = self._dreal_stream
        ex = self.exchange
        # D on the real clip needs nothing from the generator: in eager mode its forward AND backward run on a second
        # stream next to the E+G forward (whose BatchNorm / streaming kernels leave the matrix pipes idle, and vice
        # versa).  loss_D = 0.5 * (loss_fake + loss_real) is back-propagated as two halves; each parameter gradient is
        # the sum of the two contributions in either order (two addends: bitwise commutative).  The declared order of
        # the BatchNorm running-statistics updates is real first, then fake.
        if side is not None:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                pred_real = self.netD.forward_nhwc(s_nhwc)
                fwd_done = torch.cuda.Event()
                fwd_done.record(side)
                loss_real = self._gan(pred_real, True)
                loss_real.backward(self._const(0.5))                   # d(0.5 L): the factor goes in as the seed, no elementwise launches
        else:
            pred_real = self.netD.forward_nhwc(s_nhwc)
            loss_real = self._gan(pred_real, True)
        # everything above reads D only: it ran beside the previous step's G exchange + Adam(E,G) + re-pack (data parallel);
        # E / G and their gradient arena are touched from here on
        self.sync_pending_update()
        self.optimizer_G.zero_grad()
        fake, self._lc = self._generate(s_nhwc)                        # (B,F,T,1)
        self._fake = fake
        self.fake = to_nchw_view(fake)
        if side is not None:
            main.wait_event(fwd_done)                                  # running statistics: real before fake
        pred_fake = self.netD.forward_nhwc(fake.detach())
        loss_fake = self._gan(pred_fake, False)
        if side is not None:
            main.wait_stream(side)                                     # real-branch gradients are in the arena
            loss_real.record_stream(main)                              # allocated on `side`, read below on main
            ex.arm(self.arena_D, ex.plan.early_D, 1)
            loss_fake.backward(self._const(0.5))
        else:
            ex.arm(self.arena_D, ex.plan.early_D, 2)
            torch.autograd.backward([loss_fake, loss_real], [self._const(0.5), self._const(0.5)])      # d(0.5 (fake + real)): the factor as seeds
        ops.join_wgrad()
        if ex.finish(self.arena_D, ex.plan.late_D):
            main.wait_stream(ex.stream)                                # Adam(D) and the G step need the reduced D gradients
        self._loss_real, self._loss_fake = loss_real.detach(), loss_fake.detach()      # -> losses[0], losses[4] at the end of the step (one launch)

    def _seg_dupdate_gstep(self, update=True):
        if update:
            self.optimizer_D.step(1.0 / self.world)
        s = self.mel
        B, _, F, T = s.shape
        self.netD.requires_grad_(False)
        ex = self.exchange
        pred = self.netD.forward_nhwc(self._fake)
        loss_gan = self._gan(pred, True)
        loss_l1 = ops.l1_mean(self._fake, s.view(B, F, T, 1))
        # loss_G = gan + lambda_l1 * l1 (+ lambda_c * contrast) is back-propagated from its terms with the weights as seeds: the same
        # gradients bit for bit, without the scalar mul / add / ones_like launches between D's forward and the backward chain
        roots, seeds = [loss_gan, loss_l1], [self._const(1.0), self._const(self.cfg.lambda_l1)]
        if self._lc is not None:
            roots.append(self._lc)
            seeds.append(self._const(self.cfg.lambda_contrast))
        ex.arm(self.arena_G, ex.plan.early_G, 1)
        torch.autograd.backward(roots, seeds)
        ops.join_side_streams()                   # (the visual branch's flow network back-propagates on its own stream)
        if self._lc is not None:
            self.EmbeddingL2 = self._lc.detach()
        ops.join_wgrad()
        self._g_exchanged = ex.finish(self.arena_G, ex.plan.late_G)
        self.netD.requires_grad_(True)
        # the six scalars get_loss_items reports, in one launch
        check(lib().viai_step_scalars(self._loss_real.data_ptr(), self._loss_fake.data_ptr(), loss_gan.data_ptr(), loss_l1.data_ptr(),
                                      self._lc.data_ptr() if self._lc is not None else 0, float(self.cfg.lambda_l1), float(self.cfg.lambda_contrast),
                                      self.losses.data_ptr(), torch.cuda.current_stream().cuda_stream), "viai_step_scalars")
        self._scalars_src = (self._loss_real, self._loss_fake, loss_gan, loss_l1, self._lc)       # alive until the launch has run
        self._pred_fake_g = pred

    def _seg_gupdate(self):
        if self._g_exchanged and not self.use_graph:
            # Adam(E,G) + the batched weight re-pack stay on the exchange stream behind the collective; the main stream picks them
            # up at the first use of E / G in the next step (sync_pending_update)
            with torch.cuda.stream(self.exchange.stream):
                self.optimizer_G.step(1.0 / self.world)
            self.exchange.g_update_pending = True
            self._g_exchanged = False
        else:
            self.optimizer_G.step(1.0 / self.world)

    def _mutable_state(self):
        """every device tensor a train step writes and the next step reads: parameter arenas, Adam moments and step
        state, BatchNorm buffers."""
        ts = []
        for opt in (self.optimizer_G, self.optimizer_D):
            ts += [opt.arena.flat, opt.exp_avg, opt.exp_avg_sq, opt.state]
        for mod in (self.Mel_Encoder, self.Mel_Decoder, self.netD, self.VideoEncoder):
            if mod is not None:
                ts += [b for b in mod.buffers()]
        return ts

    @contextlib.contextmanager
    def _step_scope(self):
        """the ops module switches of a step: gradients land in the arenas in place (DIRECT_GRAD), weight gradients trail on this
        model's side stream as it is NOW (bench.py reassigns _wgrad_stream between steps); put back, and the gradient-ready hooks
        dropped, however the step ends"""
        prev, ops.DIRECT_GRAD = ops.DIRECT_GRAD, True
        prev_s, ops.WGRAD_STREAM = ops.WGRAD_STREAM, self._wgrad_stream
        try:
            yield
        finally:
            ops.DIRECT_GRAD, ops.WGRAD_STREAM = prev, prev_s
            ops.GRAD_HOOKS.clear()

    def optimize_parameters(self, global_step=0):
        """one G+D train step (train_whole_sync.py:76)."""
        with self._step_scope():
            if self.use_graph:
                ex = self.exchange
                self._captured.run((self._seg_forward_dstep, self._seg_dupdate_gstep, self._seg_gupdate),
                                   (lambda: ex.allreduce(self.arena_D), lambda: ex.allreduce(self.arena_G)),
                                   state=self._mutable_state, restored=self.weights_changed,
                                   avoid=(self._wgrad_stream, self._dreal_stream))
            else:
                self._seg_forward_dstep()          # D exchange: early bucket from inside the backward, the rest at its end
                self._seg_dupdate_gstep()          # G exchange: two early buckets + the encoder range
                self._seg_gupdate()
            self._stepped_since_range_check = True

    def forward_backward_no_update(self):
        """the step WITHOUT the two Adam updates (parity target, see oracle.step_no_update).  In a process group the gradient
        arenas hold the all-reduced SUMS afterwards (the 1/N lives in the Adam kernel)."""
        with self._step_scope():
            self._seg_forward_dstep()
            self._seg_dupdate_gstep(update=False)
            if self._g_exchanged:
                torch.cuda.current_stream().wait_stream(self.exchange.stream)
                self._g_exchanged = False

    def test(self):
        """forward only (train_whole_sync.py:79-80,159-183: the caller sets `model.train = 0` and wraps in no_grad).
        Runs the SAME generator path as the train step (`_generate`: with `use_video` the video feature goes through
        `deconv1_1_1`).  With `self.train == 0` the modules are put in eval mode for the call (running BatchNorm
        statistics, buffers untouched) and restored afterwards."""
        self.sync_pending_update()
        s = self.mel
        B, _, F, T = s.shape
        mods = [m for m in (self.Mel_Encoder, self.Mel_Decoder, self.VideoEncoder) if m is not None]
        was = [m.training for m in mods]
        if not self.train:
            for m in mods:
                m.eval()
        try:
            with torch.no_grad():
                fake, _lc, feats, f_v = self._generate(s.view(B, F, T, 1), want_feats=True)
                self.fake = to_nchw_view(fake)
                self._put(3, ops.l1_mean(fake, s.view(B, F, T, 1)))
                emb = feats[-1].mean(dim=(1, 2))                   # bottleneck (B, h, T/16, 256) -> (B, 256)
                self.mel_net_norm = torch.nn.functional.normalize(emb, p=2, dim=1)
                # the retrieval metrics of the reference loop (utils/util.py:99-121) pair the audio embedding with the VIDEO
                # embedding, and the loop reads `video_net_norm` unconditionally after test() (train_whole_sync.py:82-83:
                # util.to_np(model.video_net_norm)), so it is always a tensor.  Without a visual branch there is nothing to pair the
                # audio embedding with: the attribute is a zero tensor of the same shape and the retrieval numbers computed from it
                # carry no information (every "video" is equidistant from every clip).
                self.video_net_norm = (torch.nn.functional.normalize(f_v.mean(dim=(2, 3)), p=2, dim=1)
                                       if f_v is not None else torch.zeros_like(self.mel_net_norm))
        finally:
            for m, t in zip(mods, was):
                m.train(t)
        return self.fake

    # ------------------------------------------------------------ bookkeeping
    def _weight_range_check(self):
        """max |w| over both parameter arenas next to the loss scalars (same host read): the f16x2 weight images are pre-scaled by a
        static 256 and clamp beyond |w| = 255.9 -- a model that gets there has diverged, and is told so instead of training on clipped
        weights."""
        if self._wmax is None:
            self._wmax = torch.zeros(2, device=self.device)
        self._wmax.zero_()
        for i, arena in enumerate((self.arena_G, self.arena_D)):
            check(lib().viai_absmax(arena.flat.data_ptr(), arena.flat.numel(), self._wmax[i:i + 1].data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "viai_absmax")
        return self._wmax

    def get_loss_items(self):
        """host sync point (train_whole_sync.py:85).  COLLECTIVE in a data-parallel run, but only when a train step ran since the last call: train steps
        are collective themselves, so every rank gets here the same number of times; calls in the no-grad test phase (train_whole_sync.py:79-80 reads the
        losses there too, and ranks may hold unequal numbers of validation batches) and repeated reads on one rank do not communicate."""
        self.sync_pending_update()
        wr = self._weight_range_check()
        stepped, self._stepped_since_range_check = self._stepped_since_range_check, False
        if self._exchanging() and stepped:
            # data-parallel runs: the weights are replicas, so every rank should see the same maxima -- but a rank whose replica has gone bad on its own (a
            # corrupted exchange, a NaN that only its clips produce) must not raise alone and leave the others waiting in the next collective: the flag is
            # the MAX over the ranks (NaN propagates through max), one tiny all-reduce at a point where the host synchronises anyway
            from . import ddp
            wr = ddp.all_reduce_max_(torch.nan_to_num(wr, nan=float("inf"), posinf=float("inf")), self.pg)
        both = torch.cat((self.losses, wr)).tolist()
        v, wmax = both[:self.losses.numel()], both[self.losses.numel():]
        if max(wmax) > ops.F16_WEIGHT_LIMIT and os.environ.get("VIAI_F16X2", "1") != "0" and os.environ.get("VIAI_MATH", "") != "fp32":
            raise FloatingPointError("max |weight| = %.4g (E+G) / %.4g (D) is beyond %.1f, where the f16x2 weight images of the conv kernels "
                                     "clamp: the model has diverged (VIAI_F16X2=0 selects the bf16x3 kernels, which have the fp32 exponent range)"
                                     % (wmax[0], wmax[1], ops.F16_WEIGHT_LIMIT))
        self.loss_D_item, self.loss_G_item, self.loss_G_GAN_item, self.loss_mel_L1_item = v[0], v[1], v[2], v[3]
        self.reconstruct_loss_item = v[3]                      # the L1 reconstruction term (train_whole_sync.py:98 accumulates it)
        self.EmbeddingL2_item = v[5] if (self.use_video and self.cfg.lambda_contrast > 0) else 0.0
        return v

    def get_current_errors(self):
        return OrderedDict([("D", self.loss_D_item), ("G", self.loss_G_item), ("G_GAN", self.loss_G_GAN_item),
                            ("mel_L1", self.loss_mel_L1_item)])

    def get_current_visuals(self):
        out = OrderedDict()
        if self.mel is not None:
            out["real_mel"] = self.mel.detach()
            out["masked_mel"] = (self.mel * self.mask).detach()
        if self.fake is not None:
            out["fake_mel"] = self.fake.detach()
        return out

    def TF_writer(self, writer, step=0):
        if writer is None:
            return
        for k, v in self.get_current_errors().items():
            writer.add_scalar(getattr(self.hparams, "name", "viai") + "_" + k, v, step)

    def del_no_need(self):
        self._pred_fake_g = None

    def eval_model_test(self, global_step, eval_dir):
        self.test()
        os.makedirs(eval_dir, exist_ok=True)
        torch.save({"fake": self.fake.cpu(), "real": self.mel.cpu(), "mask": self.mask.cpu()},
                   os.path.join(eval_dir, "step%09d_mel.pt" % global_step))

    # ---------------------------------------------------------- checkpointing
    def save_inpainting_checkpoint(self, global_step, global_test_step, checkpoint_dir, epoch, hparams=None):
        """same dict layout as utils/util.py:146-162."""
        hp = hparams if hparams is not None else self.hparams
        self.sync_pending_update()
        path = os.path.join(checkpoint_dir, getattr(hp, "name", "viai") + "_checkpoint_step{:09d}.pth.tar".format(global_step))
        if self.world > 1 and torch.distributed.get_rank(self.pg) != 0:
            return path                                     # replicas are identical: rank 0 writes, the others do not race it
        os.makedirs(checkpoint_dir, exist_ok=True)
        keep = getattr(hp, "save_optimizer_state", True)

        def cpu_sd(m):
            return OrderedDict((k, v.detach().cpu().clone()) for k, v in m.state_dict().items())
        ck = OrderedDict([
            ("Mel_Encoder", cpu_sd(self.Mel_Encoder)), ("Mel_Decoder", cpu_sd(self.Mel_Decoder)), ("netD", cpu_sd(self.netD)),
            ("optimizer_G", self.optimizer_G.state_dict() if keep else None),
            ("optimizer_D", self.optimizer_D.state_dict() if keep else None),
            ("global_step", global_step), ("global_epoch", epoch), ("global_test_step", global_test_step),
        ])
        if self.VideoEncoder is not None:
            # utils/util.py:148 has this entry commented out -- there the visual branch was not in this optimizer; here it is
            # trained by optimizer_G (whose state dict indexes its parameters too), so a resume needs its weights and buffers
            ck["VideoEncoder"] = cpu_sd(self.VideoEncoder)
        torch.save(dict(ck), path)          # a plain dict, as utils/util.py:150 writes
        return path

    def load_inpainting_checkpoint(self, path, reset_optimizer=False):
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if self.VideoEncoder is not None and "VideoEncoder" not in ck and not reset_optimizer:
            raise KeyError("checkpoint has no 'VideoEncoder' entry: optimizer_G's moments would not belong to the freshly "
                           "initialised visual branch (pass reset_optimizer=True to load E/G/D only)")
        self.load_states(ck["Mel_Encoder"], ck["Mel_Decoder"], ck["netD"], ck.get("VideoEncoder") if self.VideoEncoder is not None else None)
        if not reset_optimizer:
            if ck.get("optimizer_G") is not None:
                self.optimizer_G.load_state_dict(ck["optimizer_G"])
            if ck.get("optimizer_D") is not None:
                self.optimizer_D.load_state_dict(ck["optimizer_D"])
        return ck["global_step"], ck["global_epoch"], ck["global_test_step"]

    def load_part_checkpoint(self, path=None):
        """tolerant partial load of E and G only (utils/util.py:124-144,165-173)."""
        path = path if path is not None else getattr(self.hparams, "resume_path", None)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        self.sync_pending_update()          # the deferred Adam(E,G) of the last step may still be writing these parameters
        for mod, key in ((self.Mel_Encoder, "Mel_Encoder"), (self.Mel_Decoder, "Mel_Decoder")):
            own = mod.state_dict()
            for k, v in ck[key].items():
                if k in own and tuple(own[k].shape) == tuple(v.shape):
                    own[k].copy_(v)
        self.weights_changed()
        return self
