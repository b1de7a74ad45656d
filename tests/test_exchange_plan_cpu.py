"""The data-parallel gradient exchange (viai_amd/exchange.py) and the step's switch scope (AudioModel._step_scope), pinned without a GPU.

  * `plan_buckets` -- which bytes of which gradient arena go to the collective, and when -- over use_video x num_D: early and late
    ranges partition each arena, every trigger lies in its own bucket, and the ranges are the ones the step has always used.
  * InstanceNorm models exchange whole arenas.
  * `GradExchange`: the hook countdown, the late ranges and the switches, with the one method that touches a stream replaced.
  * `_step_scope` puts the `ops` module switches back after a step that raises.
The networks and the arenas are built on the CPU; nothing is launched.
"""
import functools
import types

import pytest
import torch.nn as nn

from viai_amd import ops
from viai_amd.exchange import GradExchange, plan_buckets
from viai_amd.model import AudioModel, FlatArena, StepConfig
from viai_amd.networks import ImageEmbedding2, MelDecoder, MelDecoderImage, MelDiscriminator, MelEncoder, MultiScaleDiscriminator


def _named(prefix, mod):
    return [(prefix + n, p) for n, p in mod.named_parameters()]


@functools.lru_cache(maxsize=None)
def _arena_G(use_video, normlayer=None):
    """(arena, modules) of the E + G (+ V) side, named as AudioModel._build_optimizers names them"""
    hp = StepConfig()
    if normlayer is not None:
        hp.normlayer = normlayer
    mods = [MelEncoder(hp), MelDecoderImage(hp) if use_video else MelDecoder(hp)] + ([ImageEmbedding2(hp)] if use_video else [])
    return FlatArena([np for prefix, mod in zip(("E.", "G.", "V."), mods) for np in _named(prefix, mod)]), mods


@functools.lru_cache(maxsize=None)
def _arena_D(num_D):
    netD = MultiScaleDiscriminator(num_D) if num_D > 1 else MelDiscriminator()
    return FlatArena(_named("D.", netD)), [netD]


def _has_instance_norm(mods):
    return any(isinstance(m, nn.InstanceNorm2d) for mod in mods for m in mod.modules())


def _plan(use_video, num_D, normlayer=None):
    (aG, mG), (aD, mD) = _arena_G(use_video, normlayer), _arena_D(num_D)
    return plan_buckets(aG, aD, num_D, use_video, _has_instance_norm(mG), _has_instance_norm(mD)), aG, aD


G_RANGES = {     # use_video: (arena size, late, early in firing order: the convblock3 bucket first, then the head bucket)
    False: (4181888, [(0, 978752)],
            [("G.convblock3.conv3_0.weight", 3931200, 4181888), ("G.deconv1_1.weight", 978752, 3931200)]),
    True: (27975360, [(0, 978752), (4181632, 27975360)],
           [("G.convblock3.conv3_0.weight", 3930944, 4181632), ("G.deconv1_1_1.weight", 978752, 3930944)]),
}
D_RANGES = {     # num_D: (arena size, late, early)
    1: (1555072, [(0, 369792)], [("D.conv3.weight", 369792, 1555072)]),
    3: (4665216, [(0, 4665216)], []),
}


@pytest.mark.parametrize("num_D", [1, 3])
@pytest.mark.parametrize("use_video", [False, True])
def test_bucket_plan_partitions_each_arena(use_video, num_D):
    plan, aG, aD = _plan(use_video, num_D)
    for arena, early, late in ((aG, plan.early_G, plan.late_G), (aD, plan.early_D, plan.late_D)):
        ranges = sorted([(lo, hi) for _, lo, hi in early] + list(late))
        assert all(lo < hi for lo, hi in ranges)                                   # no empty range
        assert ranges[0][0] == 0 and ranges[-1][1] == arena.size
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))               # [0, size) exactly once: no gap, no overlap
        for name, lo, hi in early:
            i = arena.names.index(name)
            assert lo <= arena.offsets[i] and arena.offsets[i] + arena.params[i].numel() <= hi, name
    # the step's ranges, as they have always been
    size, late, early = G_RANGES[use_video]
    assert aG.size == size and plan.late_G == late and plan.early_G == early
    size, late, early = D_RANGES[num_D]
    assert aD.size == size and plan.late_D == late and plan.early_D == early


def test_instance_norm_models_exchange_whole_arenas():
    # a decoder built with InstanceNorm2d: no early G bucket; the D plan is the BatchNorm model's
    plan, aG, aD = _plan(False, 1, nn.InstanceNorm2d)
    assert _has_instance_norm(_arena_G(False, nn.InstanceNorm2d)[1])
    assert plan.early_G == [] and plan.late_G == [(0, aG.size)]
    assert (plan.early_D, plan.late_D) == (_plan(False, 1)[0].early_D, _plan(False, 1)[0].late_D) and plan.early_D != []
    # an InstanceNorm on the D side: the same for D, and the G plan is unaffected
    aG, aD = _arena_G(False)[0], _arena_D(1)[0]
    plan = plan_buckets(aG, aD, 1, False, instance_norm_G=False, instance_norm_D=True)
    assert plan.early_D == [] and plan.late_D == [(0, aD.size)]
    assert (plan.early_G, plan.late_G) == (_plan(False, 1)[0].early_G, _plan(False, 1)[0].late_G)


@pytest.fixture
def recorded():
    """a GradExchange at world size 2 over the num_D = 1 discriminator arena whose `_reduce` records instead of reducing"""
    plan, _aG, aD = _plan(False, 1)
    switches = types.SimpleNamespace(_skip_exchange=False, _force_allreduce=False)
    ex = GradExchange(plan, switches, pg=None, world=2, overlap=True)
    log = []
    ex._reduce = lambda arena, lo, hi, blocking=False: log.append((arena, lo, hi, blocking))
    ops.GRAD_HOOKS.clear()
    yield ex, aD, log
    ops.GRAD_HOOKS.clear()


def test_hook_fires_on_the_armed_invocation_and_finish_sends_the_late_ranges(recorded):
    ex, aD, log = recorded
    (name, lo, hi), = ex.plan.early_D
    trigger = aD.params[aD.names.index(name)]
    ex.arm(aD, ex.plan.early_D, fire_at=1)
    assert list(ops.GRAD_HOOKS) == [trigger.data_ptr()]               # keyed as ops._grad_ready looks them up
    ops._grad_ready(trigger)
    assert log == [(aD, lo, hi, False)]
    ops._grad_ready(aD.params[0])                                     # another layer's gradient: not a trigger
    assert len(log) == 1
    del log[:]
    ex.arm(aD, ex.plan.early_D, fire_at=2)                            # both halves of loss_D in one backward pass
    ops._grad_ready(trigger)
    assert log == []
    ops._grad_ready(trigger)
    assert log == [(aD, lo, hi, False)]
    del log[:]
    late = [(0, 64), (64, lo)]                                        # in the order given
    assert ex.finish(aD, late) is True
    assert log == [(aD, 0, 64, False), (aD, 64, lo, False)] and ops.GRAD_HOOKS == {}
    assert ex.stream is None and not ex.g_update_pending              # nothing here made a stream


@pytest.mark.parametrize("world,force,skip,overlap,exchanging,overlapped", [
    (2, False, False, True, True, True),
    (2, False, True, True, False, False),        # bench.py: the step without its collectives
    (1, False, False, True, False, False),
    (1, True, False, True, True, True),          # tests, probes: the exchange at world size 1
    (1, True, True, True, False, False),
    (2, False, False, False, True, False),       # graph mode: whole arenas between the captured segments
])
def test_switches_are_read_at_every_call(recorded, world, force, skip, overlap, exchanging, overlapped):
    ex, aD, log = recorded
    ex.world, ex.overlap = world, overlap
    ops.GRAD_HOOKS[0] = lambda: None                                  # a stale hook: arm() and finish() drop it either way
    ex.switches._force_allreduce, ex.switches._skip_exchange = force, skip       # set after construction, as bench.py and the probes do
    assert (ex.exchanging(), ex.overlapped()) == (exchanging, overlapped)
    ex.arm(aD, ex.plan.early_D, 1)
    assert len(ops.GRAD_HOOKS) == (1 if overlapped else 0) and 0 not in ops.GRAD_HOOKS
    assert ex.finish(aD, ex.plan.late_D) is overlapped
    assert log == ([(aD,) + ex.plan.late_D[0] + (False,)] if overlapped else []) and ops.GRAD_HOOKS == {}
    del log[:]
    ex.allreduce(aD)
    assert log == ([(aD, 0, aD.size, True)] if exchanging else [])


def test_step_scope_restores_the_switches_after_a_step_that_raises():
    m = AudioModel.__new__(AudioModel)            # no device: only the attribute the scope reads
    m._wgrad_stream = stream = object()
    before = (ops.DIRECT_GRAD, ops.WGRAD_STREAM)
    ops.DIRECT_GRAD, ops.WGRAD_STREAM = was = (object(), object())
    try:
        with pytest.raises(ZeroDivisionError):
            with m._step_scope():
                assert ops.DIRECT_GRAD is True and ops.WGRAD_STREAM is stream
                ops.GRAD_HOOKS[1] = lambda: None
                1 / 0
        assert (ops.DIRECT_GRAD, ops.WGRAD_STREAM) == was and ops.GRAD_HOOKS == {}
        m._wgrad_stream = None                    # reassigned between steps (bench.py): the next step sees the new value
        with m._step_scope():
            assert ops.WGRAD_STREAM is None
        assert (ops.DIRECT_GRAD, ops.WGRAD_STREAM) == was
    finally:
        ops.DIRECT_GRAD, ops.WGRAD_STREAM = before
        ops.GRAD_HOOKS.clear()
