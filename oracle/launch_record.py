"""Launch recorder (checker only; the product never imports it): which conv4x4 / wgrad4x4 / normalisation launches a training step
issues, with every descriptor field, so that tests/test_step_launches_gpu.py can replay each one on fresh buffers against
oracle/launch_ref.py.

`record()` monkeypatches vts.ops._run.  For every call of a recorded C entry it keeps a copy of the descriptor (pointers as plain
integers: the replay needs whether one is set and its alignment, and the recorder links calls through them), the in / out value of
`fused` / `slots`, the scratch size and vts_last_kernel() after the call.  Host-only work: it may run while a HIP graph is being
captured, which is where the benchmarked schedule is dispatched."""
import contextlib
import ctypes as C

ENTRIES = ("vts_conv4x4", "vts_conv4x4_norm", "vts_conv4x4_bsums", "vts_wgrad4x4", "vts_norm_stats", "vts_norm_bwd",
           "vts_norm_stats_from_partials", "vts_norm_bwd_from_partials", "vts_wgrad_reduce_batch")


def to_py(v):
    """ctypes value -> plain python (Structure -> dict, array -> tuple); pointers become ints (0 = NULL)"""
    if isinstance(v, C.Structure):
        return {name: to_py(getattr(v, name)) for name, _ in v._fields_}
    if isinstance(v, C.Array):
        return tuple(to_py(x) for x in v)
    if v is None:
        return 0
    return v


def to_c(cls, d):
    """inverse of to_py for a Structure class"""
    s = cls()
    for name, typ in cls._fields_:
        v = d[name]
        if isinstance(typ, type) and issubclass(typ, C.Structure):
            setattr(s, name, to_c(typ, v))
        elif isinstance(typ, type) and issubclass(typ, C.Array):
            arr = getattr(s, name)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(s, name, v)
    return s


# pointer fields: in a signature they only say whether they are set and how they are aligned
_PTR = {"data", "scale", "shift", "w", "bias", "out", "ws", "dw", "x", "gamma", "beta", "running_mean", "running_var",
        "num_batches_tracked", "mean_out", "rstd_out", "counters", "stat_mean_out", "stat_uvar_out", "ext_mean", "ext_uvar", "dy",
        "mean", "rstd", "dgamma", "dbeta"}


def signature(d):
    """hashable form of a descriptor dict with every pointer reduced to -1 (NULL) or its address mod 16 (kernels take vector paths
    by alignment)"""
    if isinstance(d, dict):
        return tuple((k, (v % 16 if v else -1) if k in _PTR else signature(v)) for k, v in d.items())
    if isinstance(d, (tuple, list)):
        return tuple(signature(x) for x in d)
    return d


class Recorder:
    def __init__(self):
        self.calls = []          # one dict per recorded call, in issue order
        self._ws_owner = {}      # deferred wgrad partial pointer -> index of the wgrad call that wrote it
        self._bsums = {}         # (out pointer, part pointer) -> index of the bsums call that left sums for a norm backward

    def hook(self, orig):
        from vts import lib as L

        def run(label, nbytes, flops, fn, *args):
            name = getattr(fn, "__name__", "")
            if name not in ENTRIES:
                return orig(label, nbytes, flops, fn, *args)
            rec = {"fn": name}
            if name == "vts_wgrad_reduce_batch":
                jobs = [to_py(j) for j in args[0]]
                rec["jobs"] = jobs
                rec["seg_calls"] = [[self._ws_owner.pop(j["part"][s]) for s in range(j["nseg"])] for j in jobs]
            else:
                rec["desc"] = to_py(args[0]._obj)
            if name in ("vts_conv4x4_norm",):
                rec["nd"] = to_py(args[1]._obj)
                rec["stat_ws_floats"] = int(args[3])
                rec["fused_in"] = args[4]._obj.value
            if name == "vts_conv4x4_bsums":
                rec["part_floats"] = int(args[2])
                rec["slots_in"] = args[3]._obj.value
            if name in ("vts_norm_stats_from_partials", "vts_norm_bwd_from_partials"):
                rec["slots"] = int(args[2])
            if name == "vts_norm_bwd_from_partials":
                rec["beta"] = int(args[3] or 0)
            orig(label, nbytes, flops, fn, *args)
            rec["kernel"] = L.load().vts_last_kernel().decode()
            idx = len(self.calls)
            if name == "vts_conv4x4_norm":
                rec["fused"] = args[4]._obj.value
            elif name == "vts_conv4x4_bsums":
                rec["slots"] = args[3]._obj.value
                if rec["slots"] > 0:
                    self._bsums[(rec["desc"]["out"], int(args[1]))] = idx
            elif name == "vts_wgrad4x4" and rec["desc"]["defer"]:
                self._ws_owner[int(args[1])] = idx
            elif name == "vts_norm_stats_from_partials":
                prev = self.calls[-1]          # ops.conv4x4 issues the merge right behind its convolution
                assert prev["fn"] == "vts_conv4x4_norm" and prev["fused"] == rec["slots"] + 2, prev
                rec["parent"] = idx - 1
            elif name == "vts_norm_bwd_from_partials":
                rec["parent"] = self._bsums.pop((rec["desc"]["dy"], int(args[1])))
            self.calls.append(rec)

        return run


@contextlib.contextmanager
def record():
    from vts import ops

    rec = Recorder()
    orig = ops._run
    ops._run = rec.hook(orig)
    try:
        yield rec
    finally:
        ops._run = orig
