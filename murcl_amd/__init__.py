"""murcl_amd: MI355X-native hot path of MuRCL (MIL aggregators, NT-Xent, PPO sub-bag sampler).

Python mirrors of the reference's modules live in murcl_amd.models / murcl_amd.utils with the
reference's class names, constructor arguments, return tuples and state-dict keys; all tensor
math inside them runs in hand-written gfx950 HIP kernels loaded from libmurcl_amd.so
(C-ABI: include/murcl_amd.h).  There is no CPU fallback.
"""
__version__ = "0.1.0"

import contextlib as _contextlib


def set_deterministic(flag):
    """Turn deterministic mode on or off for the whole process -> the previous state.  While it is on, every kernel launch takes
    a form whose float sums are added in a fixed order (per-split partial results to a workspace, then one reduce launch): same
    device, same build, same shapes, same CU budget, same seed -> the same bits, in outputs, gradients and optimizer steps.  The
    mode is read when a kernel is launched (forward and backward alike); a captured graph keeps the form it was captured with."""
    from . import _lib
    return bool(_lib.lib().murcl_set_deterministic(int(bool(flag))))


def is_deterministic():
    from . import _lib
    return bool(_lib.lib().murcl_deterministic())


@_contextlib.contextmanager
def deterministic(flag=True):
    """``with murcl_amd.deterministic(): ...`` - the mode inside the block, the previous state afterwards (also on an exception)."""
    prev = set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(prev)
