"""Experiment switches of the Python layer: the ones a test or bench.py drives (the serial / joined / chained schedules, lane packing,
the fresh-batch paths, the kernel-family forms compared bit for bit) and the measuring instruments (VTS_KO_LANES, VTS_KNOCKOUT, which
knowingly break the arithmetic for timing experiments).  README.md "Switches" lists them all.  Switches whose variant was measured,
lost and written up (profiles/HISTORY.md, profiles/r06a_experiments.md) are retired: the code runs the winner.

None is a user option, so they are read from
the environment ONLY while VTS_TUNING=1 is set: without it every switch has its measured default and a stray VTS_* variable in a user's
shell changes nothing.  (The C library has the same rule at compile time: csrc/vts_internal.h:vts_tune, make PROFILING=1.)

What a user may set, always honoured: VTS_LIB_PATH (another build of the library), VTS_DDP_BACKEND / VTS_DDP_DIRECT / VTS_DDP_FORCE /
VTS_G_BUCKETS / VTS_G_BUCKET_MIN_MB (data parallel), VTS_{LPIPS,LPIPS_ALEX,VGG,INCEPTION}_WEIGHTS (weight files), VTS_SIFID,
VTS_LPIPS_METRICS (optional metrics), VTS_RCCL_LIB (C library)."""
import os


def on():
    return os.environ.get("VTS_TUNING", "0") == "1"


def get(name, default):
    """the environment's value of an experiment switch while VTS_TUNING=1, else `default`"""
    return os.environ.get(name, default) if on() else default


def is_set(name):
    return on() and bool(os.environ.get(name))
