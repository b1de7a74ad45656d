"""The data-parallel gradient exchange of the train step: which bytes of which gradient arena go to RCCL, and when.

`plan_buckets` is arithmetic on parameter names and offsets (no device).  `GradExchange` runs a plan: it arms the gradient-ready
hooks (ops.GRAD_HOOKS) that hand the early buckets to the collective from inside the backward pass, sends the late ranges after
it, and keeps the one piece of state that outlives a step -- whether the G exchange + Adam(E,G) + re-pack of the previous step
are still on the exchange stream.  model.AudioModel decides the order of operations; nothing here launches a kernel.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops

# early_*: [(trigger parameter name, lo, hi)] in the order the backward completes them;  late_*: [(lo, hi)]
BucketPlan = namedtuple("BucketPlan", "early_G late_G early_D late_D")


def plan_buckets(arena_G, arena_D, num_D=1, use_video=False, instance_norm_G=False, instance_norm_D=False):
    """Gradient buckets of the data-parallel exchange: contiguous ranges of the flat gradient arenas in the order the
    backward pass completes them.  An EARLY bucket (trigger parameter, lo, hi) goes to RCCL from a gradient-ready hook
    (ops.GRAD_HOOKS) as soon as the layer owning the trigger has queued its gradients -- the rest of the backward chain
    runs beside the collective; the LATE ranges follow after the last weight gradient.
      D  (6.2 MB):  early [conv3.weight .. end) = conv3 + norm3 + conv4, 76 % of the bytes, ready after the second layer of
                    the backward chain;  late [0 .. conv3.weight)
      G (16.7 MB):  early [convblock3 .. end of G), then [G start .. convblock3) at deconv1_1;  late = E (+ the visual branch).
    The G exchange, Adam(E,G) and the weight re-pack stay on the exchange stream and overlap the NEXT step's D(real) forward +
    backward, which reads none of them (see AudioModel._seg_forward_dstep).

    `arena_*`: anything with the `names`, `offsets` and `size` of a model.FlatArena whose names carry the prefixes E. / G. / V. /
    D. (AudioModel._build_optimizers).  `instance_norm_*`: that side of the model holds an nn.InstanceNorm2d."""
    aD, aG = arena_D, arena_G

    def off(arena, name):
        return arena.offsets[arena.names.index(name)]
    early_D, late_D = [], [(0, aD.size)]
    if num_D == 1:
        o = off(aD, "D.conv3.weight")
        early_D, late_D = [("D.conv3.weight", o, aD.size)], [(0, o)]
    g_lo = off(aG, next(n for n in aG.names if n.startswith("G.")))
    v_names = [n for n in aG.names if n.startswith("V.")]
    g_hi = off(aG, v_names[0]) if v_names else aG.size
    c3 = off(aG, "G.convblock3.conv3_0.weight")
    head = "G.deconv1_1_1.weight" if use_video else "G.deconv1_1.weight"
    early_G = [("G.convblock3.conv3_0.weight", c3, g_hi), (head, g_lo, c3)]
    late_G = [(0, g_lo)] + ([(g_hi, aG.size)] if g_hi < aG.size else [])
    # An InstanceNorm2d layer runs conv_bn_act once PER SAMPLE with the same weight (networks._instance_norm_layer): the trigger
    # layer's backward is then invoked B times per pass and a hook armed for one invocation would hand the bucket to RCCL while the
    # other samples are still accumulating into it.  Such models exchange each arena whole, after its last weight gradient.
    if instance_norm_D:
        early_D, late_D = [], [(0, aD.size)]
    if instance_norm_G:
        early_G, late_G = [], [(0, aG.size)]
    return BucketPlan(early_G, late_G, early_D, late_D)


class GradExchange:
    """Runs a BucketPlan over a process group.

    `switches` is the object that carries the two run-time switches, `_skip_exchange` (bench.py: the step without its collectives)
    and `_force_allreduce` (tests, probes: exchange even at world size 1).  They are set from outside between steps, so they are
    read at every call, never copied.  `overlap`: the bucketed exchange from inside the step (eager mode); without it the caller
    exchanges whole arenas between its captured segments (`allreduce`).

    Every collective, and every use of the exchange stream by this class but `sync_pending_update`, is in `_reduce`: with that
    one method replaced the rest runs on the host alone."""

    def __init__(self, plan, switches, pg=None, world=1, overlap=True, device=None):
        self.plan, self.switches = plan, switches
        self.pg, self.world, self.overlap, self.device = pg, world, overlap, device
        self.stream = None                 # data-parallel exchange stream (created on first use)
        self.g_update_pending = False      # the G exchange + Adam(G) + re-pack of the previous step are still on `stream`

    def exchanging(self):
        return (self.world > 1 or self.switches._force_allreduce) and not self.switches._skip_exchange

    def overlapped(self):
        """bucketed exchange from inside the step (eager mode); graph mode exchanges between its captured segments instead"""
        return self.exchanging() and self.overlap

    def _reduce(self, arena, lo, hi, blocking=False):
        """sum-all-reduce of arena.grad[lo:hi] on the exchange stream, behind everything queued so far on the current stream
        and on the weight-gradient stream (in-place on the arena: no packing copies).  `blocking`: on the current stream instead."""
        from . import ddp
        if blocking:
            ddp.all_reduce_sum_(arena.grad[lo:hi], self.pg)
            return
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        comm = self.stream
        comm.wait_stream(torch.cuda.current_stream())
        if ops.WGRAD_STREAM is not None:
            comm.wait_stream(ops.WGRAD_STREAM)
        with torch.cuda.stream(comm):
            ddp.all_reduce_sum_(arena.grad[lo:hi], self.pg)

    def arm(self, arena, early, fire_at=1):
        """register the early buckets of `arena` as gradient-ready hooks; `fire_at` = which invocation of the trigger layer's
        backward completes its gradient (2 when both halves of loss_D are back-propagated in one pass)."""
        ops.GRAD_HOOKS.clear()
        if not self.overlapped():
            return
        for name, lo, hi in early:
            p = arena.params[arena.names.index(name)]
            state = {"n": fire_at}

            def hook(state=state, lo=lo, hi=hi):
                state["n"] -= 1
                if state["n"] == 0:
                    self._reduce(arena, lo, hi)
            ops.GRAD_HOOKS[p.data_ptr()] = hook

    def finish(self, arena, late):
        """after the backward pass: the late ranges.  True: the reduced gradients are on the exchange stream, and whoever needs them
        waits for it."""
        ops.GRAD_HOOKS.clear()
        if not self.overlapped():
            return False
        for lo, hi in late:
            self._reduce(arena, lo, hi)
        return True

    def allreduce(self, arena):
        """graph mode only: blocking whole-arena exchange between the captured segments."""
        if self.exchanging():
            self._reduce(arena, 0, arena.size, blocking=True)

    def sync_pending_update(self):
        """the main stream waits for the deferred G exchange + Adam(E,G) + re-pack of the previous step (no host sync).  Called at
        the point of the next step that first touches E / G, and by everything that reads parameters between steps."""
        if self.g_update_pending:
            torch.cuda.current_stream().wait_stream(self.stream)
            self.g_update_pending = False
