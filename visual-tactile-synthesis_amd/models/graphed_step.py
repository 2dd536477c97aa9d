"""GraphedStepModel: the training-step scaffold the four models share, on our side of the BaseModel boundary (nothing in the reference
corresponds to it).

A model cuts its step into segments (`_segments`: plain callables that launch kernels on persistent buffers) and calls `_run_step()` from
optimize_parameters after its own preamble.  The first step runs the segments eagerly; from the second on they are captured once as HIP
graphs on one memory pool and replayed, with the gradient buckets of a data-parallel run waited for and started between them.  This class
owns what that takes: the loss-slot buffer, the persistent input buffers, capture and drop of the graphs (with the workspace hold that
keeps their scratch memory in place), and the host mirrors of the optimisers' step counters.
"""
import torch

from vts import ops

from .base_model import BaseModel


class GraphedStepModel(BaseModel):
    LOSS_SLOTS = ()     # names of the loss slots, in buffer order: get_current_losses sets loss_<name> of every one

    def _init_step_state(self):
        """called once from the subclass's __init__"""
        self._loss_buf = ops.loss_slots(len(self.LOSS_SLOTS), self.device)     # int64 fixed point (order-independent accumulation)
        self._slot = {n: self._loss_buf[i:i + 1] for i, n in enumerate(self.LOSS_SLOTS)}
        self._bufs = {}         # persistent input buffers (stable addresses for captured HIP graphs)
        self._graphs = None     # the captured segments of the step, or None
        self.graph_nodes = None     # (all nodes, kernel nodes) per captured segment
        self._eager_steps_done = 0
        self.ddp = None

    # ------------------------------------------------------------------ input
    def _drop_graphs(self):
        if self._graphs is not None:
            self._graphs = None
            ops.release_ws((id(self), "train"))

    def _load(self, name, host):
        """host array -> persistent float32 device buffer; a shape change re-allocates it and invalidates the graphs"""
        t = torch.as_tensor(host)
        buf = self._bufs.get(name)
        if buf is None or tuple(buf.shape) != tuple(t.shape):
            buf = self._bufs[name] = torch.empty(tuple(t.shape), dtype=torch.float32, device=self.device)
            self._drop_graphs()
        buf.copy_(t.to(torch.float32), non_blocking=True)
        return buf

    # ------------------------------------------------------------------ training step
    def _segments(self):
        """[(segment, gradient buckets to wait for before it, buckets to start after it)]"""
        raise NotImplementedError

    def _may_use_graphs(self):
        return bool(getattr(self.opt, "use_hip_graph", False))

    def _after_capture(self):
        pass

    def _after_step(self, replay, use_graph):
        pass

    def _comm(self, name, start):
        if self.ddp is None or name not in self.ddp.buckets:
            return
        b = self.ddp.buckets[name]
        b.start() if start else b.wait()

    def _capture_graphs(self):
        """Capture the segments as HIP graphs sharing one memory pool (torch.cuda.CUDAGraph over the launch stream our ctypes kernels
        use).  Capturing records work without executing it."""
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        stream = torch.cuda.Stream()
        counts = [o.step_count for o in self.optimizers]
        graphs, nodes = [], []
        ops.freeze_ws((id(self), "train"))
        try:
            for seg, _, _ in self._segments():
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, stream=stream, capture_error_mode="thread_local"):   # RCCL's watchdog thread queries events meanwhile
                    seg()
                    nodes.append(ops.capture_node_count())      # (all nodes, kernel nodes) of this segment: the replayed launch count
                graphs.append(g)
        except Exception:
            ops.release_ws((id(self), "train"))
            raise
        for o, c in zip(self.optimizers, counts):
            o.step_count = c   # host mirrors moved during capture; the device counters did not
        self._graphs = graphs
        self.graph_nodes = nodes
        self._after_capture()

    def _run_step(self):
        """one training step: eager the first time, then captured (once) and replayed"""
        self._gscale = self.ddp.grad_scale if self.ddp is not None else 1.0
        for o in self.optimizers:
            o.sync_lr()
        use_graph = self._may_use_graphs()
        if use_graph and self._graphs is None and self._eager_steps_done >= 1:
            self._capture_graphs()
        replay = use_graph and self._graphs is not None
        for i, (seg, wait_for, start_after) in enumerate(self._segments()):
            for nme in wait_for:
                self._comm(nme, start=False)
            if replay:
                self._graphs[i].replay()
            else:
                seg()
            for nme in start_after:
                self._comm(nme, start=True)
        if replay:
            for o in self.optimizers:
                o.step_count += 1
        else:
            self._eager_steps_done += 1
        self._after_step(replay, use_graph)

    # ------------------------------------------------------------------ logging
    def get_current_losses(self):
        vals = ops.loss_values(self._loss_buf)   # the only device->host sync of the loss path
        for i, name in enumerate(self.LOSS_SLOTS):
            setattr(self, "loss_" + name, vals[i])
        return BaseModel.get_current_losses(self)
