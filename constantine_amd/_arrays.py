"""What every ctypes caller of the package does with its arrays: numpy uint8 buffers on the host, torch CUDA tensors or raw addresses
on the device."""
import ctypes

import numpy as np


def is_cuda(a):
    """is `a` a torch CUDA tensor"""
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def ptr(a):
    """`a` as a void* argument: a torch tensor, a numpy array, None (NULL) or a raw integer address"""
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr())
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return None if a is None else ctypes.c_void_p(int(a))


def result_buffer(info, coord):
    """a zeroed host buffer for one point of `info`'s curve: 2 coordinates for "aff", 3 for "jac" / "prj" """
    return np.zeros((2 if coord == "aff" else 3) * info.coord_bytes, dtype=np.uint8)


def order(L, ctx, *arrays):
    """Order the engine's stream after torch's current stream when an argument is a torch CUDA tensor (the first one decides): the
    engine runs on its own non-blocking streams, so without this a kernel that is still producing the tensor could be overtaken
    (ctt_hip_msm_wait_stream; INTEGRATION.md "Stream ordering").  Raw integer addresses carry no stream: their owner orders them
    (DeviceMsm.wait_stream / a synchronize)."""
    for a in arrays:
        if is_cuda(a):
            import torch
            s = torch.cuda.current_stream(a.device)
            # Nothing in flight on the producer stream: whatever wrote the tensors is done, and there is nothing to order against.
            # (The event record + two stream waits per submit are a barrier packet on the producer's queue and ~10 us of host
            # time -- a pipelined caller of small MSMs whose producer is torch's legacy null stream measured 0.67 -> 0.80 ms per MSM at
            # 2^17 pairs with three MSMs in flight because of them; the query is one hipStreamQuery.)
            if not s.query() and L.ctt_hip_msm_wait_stream(ctx, ctypes.c_void_p(s.cuda_stream)) != 0:
                raise RuntimeError("ctt_hip_msm_wait_stream failed")
            return
