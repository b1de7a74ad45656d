"""The train step captured once and replayed: three hipGraphs, or three launch plans (csrc/plan.hip), split at the two gradient
all-reduce points.

`CapturedStep` owns what a capture produces -- the graphs, the plans, the scratch buffers of the graphs' private pool -- and their
lifetime: nothing is destroyed while it may still be replaying, and nothing is destroyed (no device synchronisation) while another
capture is in progress.  It holds no reference to the model: the segment callables are bound methods of the model, and a model
that could only be freed by the cycle collector would keep its plans, and its device memory, for as long as that takes.  So the
model hands them over with every run().
"""
from __future__ import annotations

import ctypes

import torch

from . import ops
from ._lib import check, load as lib

_PARKED_PLANS = []      # launch plans of models that were collected while a stream capture was in progress (see CapturedStep.close)


class CapturedStep:
    def __init__(self, device, use_plan=False):
        """use_plan: the step is stream-captured once and replayed from C as a launch plan (csrc/plan.hip): the eager step's
        kernels, arguments, streams and cross-stream edges without the per-launch host work."""
        self.device, self.use_plan = device, bool(use_plan)
        self._graphs = None
        self._plans = None
        self._graph_scratch = None

    def run(self, segs, between, state, restored, avoid):
        """replay segs[0], between[0]() (the D exchange), segs[1], between[1]() (the G exchange), segs[2]; captures first when
        there is nothing to replay.  For the capture: `state()` lists every device tensor a step writes and the next step reads,
        `restored()` runs once they have been put back after the warm-up, `avoid` are the streams (or None) the segments fork
        onto, which the capture must not originate on."""
        if self._graphs is None:
            self._capture(segs, state, restored, avoid)
        if self.use_plan:
            run = [lambda p=p: check(lib().viai_plan_replay(p, torch.cuda.current_stream().cuda_stream), "viai_plan_replay")
                   for p in self._plans]
        else:
            run = [g.replay for g in self._graphs]
        run[0]()
        between[0]()
        run[1]()
        between[1]()
        run[2]()

    def _capture(self, segs, state, restored, avoid):
        """three HIP graphs split at the two gradient all-reduce points."""
        # Warm-up on a side stream (allocator + lazy init).  The warm-up runs two REAL steps (both Adam updates, the
        # BatchNorm running statistics) without any gradient exchange, so everything a step mutates is snapshotted first
        # and put back afterwards: a (re-)capture -- first step, or a new input shape -- then leaves parameters, Adam
        # moments / step counters and BatchNorm buffers exactly where they were, on every rank.
        snap = state()
        saved = [t.clone() for t in snap]
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for _ in range(2):
                for f in segs:
                    f()
        torch.cuda.current_stream().wait_stream(st)
        for t, v in zip(snap, saved):
            t.copy_(v)
        restored()
        graphs, plans = [], []
        pool = None
        before = ops.scratch_snapshot()
        # torch hands out streams from a pool of 32 per device, round robin, and torch.cuda.graph's default capture stream is one pool
        # stream made once per process: in a long-lived process it can be the very stream this model got as a side stream, and the
        # captured branch would collapse into the origin.  Capture on a stream known to differ from both side streams.
        taken = {st.cuda_stream for st in avoid if st is not None}
        cap = torch.cuda.Stream(device=self.device)
        while cap.cuda_stream in taken:
            cap = torch.cuda.Stream(device=self.device)
        # With a process group up, ProcessGroupNCCL's watchdog THREAD polls its work events (hipEventQuery) whenever it likes; under the default
        # capture mode ("global") that call is illegal from any thread while this one captures, the watchdog dies with
        # hipErrorStreamCaptureUnsupported and takes the process with it -- the "RCCL abort now and then" of rounds 2 and 3 (1 of 20 runs of the
        # one-rank test; it was never RCCL's set-up or teardown).  "thread_local" confines the check to the capturing thread.
        dist_up = torch.distributed.is_available() and torch.distributed.is_initialized()
        gkw = {"capture_error_mode": "thread_local"} if dist_up else {}
        for f in segs:
            if self.use_plan:
                # the capture is a recorder: the hipGraph is kept (it owns the kernel-argument arrays) but never instantiated
                g = torch.cuda.CUDAGraph(keep_graph=True)
                check(lib().viai_plan_log_begin(), "viai_plan_log_begin")
                try:
                    with torch.cuda.graph(g, pool=pool, stream=cap, **gkw):
                        origin = torch.cuda.current_stream().cuda_stream
                        f()
                finally:
                    lib().viai_plan_log_end()
                plan = ctypes.c_void_p()
                check(lib().viai_plan_build(int(g.raw_cuda_graph()), origin, ctypes.byref(plan)), "viai_plan_build")
                plans.append(plan)
            else:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, stream=cap, **gkw):
                    f()
            pool = g.pool()
            graphs.append(g)
        self._graphs = graphs
        self._plans = plans if self.use_plan else None
        # scratch buffers first requested inside the captures came from the graphs' private pool: they belong to this object now
        self._graph_scratch = ops.scratch_take_new(before)

    def drop(self):
        """new input shape: the captured graphs are stale.  They may still be replaying (steps are asynchronous) and a hipGraphExec
        must not be destroyed while in flight, so this is one of the few places that waits for the device."""
        if self._graphs is not None:
            torch.cuda.synchronize(self.device)
            if self._plans is not None:
                for p in self._plans:
                    lib().viai_plan_destroy(p)
                self._plans = None
            self._graphs = None
            self._graph_scratch = None
            ops.drop_scratch()            # scratch buffers allocated while capturing live in the dead graphs' private memory pool

    def close(self):
        """release what the launch plans hold (events, plan nodes).  Also runs from the model's __del__, i.e. whenever the garbage
        collector gets to a dropped model -- possibly in the middle of ANOTHER model's stream capture, where a device synchronisation
        would invalidate that capture: plans are then parked and destroyed at the next close() outside a capture.  The process-wide
        scratch pool is not touched from here (buffers a capture of THIS step allocated live in self._graph_scratch and go with the
        object)."""
        plans, self._plans = (self._plans or []), None
        self._graphs = None
        self._graph_scratch = None
        if not plans and not _PARKED_PLANS:
            return
        try:
            if torch.cuda.is_current_stream_capturing():
                _PARKED_PLANS.extend(plans)
                return
            torch.cuda.synchronize(self.device)         # a plan's events / kernel nodes must not be destroyed while a replay is in flight
            for p in plans + _PARKED_PLANS:
                lib().viai_plan_destroy(p)
            del _PARKED_PLANS[:]
        except Exception:
            pass                                        # interpreter shutdown: the driver is gone, nothing left to release

    def plan_info(self):
        """per captured segment: nodes, kernels, kernels with a noted stream, copies, fills, streams, events, waits"""
        out = []
        for p in self._plans or ():
            v = (ctypes.c_int * 8)()
            check(lib().viai_plan_info(p, v, 8), "viai_plan_info")
            out.append(list(v))
        return out
