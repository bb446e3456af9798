"""Host plumbing the scan loaders share (kittiprep.py, nuscprep.py; scanprep.py takes ``out_rows``).  ``name``: the caller's entry
point, the prefix of every message; ``call``: the caller's own ``call``, so that whoever wraps a loader's ``call`` sees every entry."""
import numpy as np
import torch

from ._lib import host_addr, host_i32, host_ptrs, ptr, stream


def image_size_wh(name, image_size):
    try:
        w, h = (int(v) for v in image_size)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: image_size must be (W, H), got {image_size!r}") from None
    if w <= 0 or h <= 0 or w >= 1 << 24 or h >= 1 << 24:
        raise ValueError(f"{name}: image_size must be (W, H) with positive sides, got {image_size!r}")
    return w, h


def tensor_checker(name):
    """-> (tensor(b, sample, key, dtypes, what): the tensor after the type and dtype checks, the (key, tensor) pairs it has seen)"""
    seen = []

    def tensor(b, s, key, dtypes, what):
        t = s.get(key)
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {key} of sample {b} must be a torch tensor on the GPU, got {type(t).__name__}")
        if t.dtype not in dtypes:
            raise TypeError(f"{name}: {key} must be {what}, got {t.dtype}")
        seen.append((key, t))
        return t
    return tensor, seen


def check_devices(name, seen):
    """Last, so that a malformed call is named as such on any device."""
    for key, t in seen:
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {key} must be on the GPU (there is no CPU fallback)")
        if t.device != seen[0][1].device:
            raise ValueError(f"{name}: {key} is on {t.device}; all tensors of a call must be on one device")


def out_rows(n, *shape, dtype=torch.float32, device=None):
    """(tensor of n rows, bytes per row, address): never a null address, also when every row was dropped"""
    t = torch.empty(max(n, 1), *shape, dtype=dtype, device=device)
    return t[:n], t.stride(0) * t.element_size(), t.data_ptr()


def ground_mask(call, g_indices, n):
    """The index lists of a chunk's scans (n: its host_i32 row counts) -> (gmask (sum n,) uint8 over the chunk's flat raw rows,
    bad (1,) int32: the indices outside their scan), numpy's indexing."""
    g = [t.contiguous() for t in g_indices]
    gmask = torch.empty(max(sum(n), 1), dtype=torch.uint8, device=g[0].device)
    bad = torch.empty(1, dtype=torch.int32, device=g[0].device)
    gt, gn = host_ptrs(g), host_i32([t.numel() for t in g])
    call("mopa_kittiprep_ground", host_addr(gt), host_addr(gn), host_addr(n), len(g), ptr(gmask), ptr(bad), stream())
    return gmask, bad


def read_counts(name, chunks, per_scan):
    """The one blocking read-back of a call: every chunk's counts (per_scan int64 per scan, then the ground indices outside their
    scan) -> (B, per_scan) int64 numpy array."""
    host = (chunks[0]["counts"] if len(chunks) == 1 else torch.cat([c["counts"] for c in chunks])).cpu().numpy()
    counts = np.zeros((chunks[-1]["e"], per_scan), dtype=np.int64)
    at = 0
    for c in chunks:
        k = per_scan * c["B"]
        counts[c["s"]:c["e"]] = host[at:at + k].reshape(-1, per_scan)
        if host[at + k]:
            raise IndexError(f"{name}: g_indices of samples {c['s']}..{c['e'] - 1} hold {int(host[at + k])} indices outside their scan")
        at += k + 1
    return counts
