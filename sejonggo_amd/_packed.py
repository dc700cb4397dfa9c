"""What the record analyses (tactics, life, shapes, moves, influence) share on the Python side: bitsets as point lists, and the
opening of their module-level entry `name(size, records, index=None, ...)`."""
import numpy as np


def points(words, N):
    """the ascending list of the set points of a bitset of uint32 words"""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:N]
    return [int(a) for a in np.flatnonzero(bits)]


def device_records(size, records, index, error=AssertionError):
    """(records, R, idx, n): packed records (a numpy array or a tensor, [R, 16 * NW] 32-bit words) as a contiguous int32 tensor on
    the current device, their number, `index` as a device tensor (None: every record in order) and the number of rows asked."""
    import torch
    from . import _lib
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    if not torch.is_tensor(records):
        records = torch.from_numpy(np.ascontiguousarray(records).view(np.int32))
    records = records.to(dev).contiguous()
    if records.dim() != 2 or int(records.shape[1]) != lib.sgo_packed_words(size):
        raise error("records must be [R, 16 * NW] words")
    idx = None if index is None else torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
    R = int(records.shape[0])
    return records, R, idx, R if idx is None else int(idx.shape[0])
