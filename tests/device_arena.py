"""Guard-band arena for tests that call the C ABI on raw device pointers (shared by
test_tgv_gpu.py and test_vector_ops_gpu.py)."""
import numpy as np

GUARD = 64                          # elements before and after every array
SENTINEL = 12345.0


class Arena(object):
    """Device arrays inside one allocation, each with GUARD sentinel elements before and
    after it.  offset: elements by which every array is shifted off 16-byte alignment.
    last: the name of the array that ends exactly where the allocation ends."""

    def __init__(self, arrays, dtype, offset=0, last=None):
        import torch
        from nsol_amd.device import to_device
        names = [k for k in arrays if k != last] + ([last] if last else [])
        pos, at = GUARD + offset, {}
        for k in names:
            at[k] = pos
            size = arrays[k].size
            pos += size + GUARD
            pos += (-pos) % 4 + offset             # starts: 16-byte aligned + offset
        total = at[last] + arrays[last].size if last else pos
        host = np.full(total, SENTINEL, dtype=dtype)
        self.mask = np.ones(total, dtype=bool)     # True: guard
        for k in names:
            host[at[k]:at[k] + arrays[k].size] = arrays[k].reshape(-1)
            self.mask[at[k]:at[k] + arrays[k].size] = False
        self.dtype, self.at, self.sizes = dtype, at, {k: arrays[k].size for k in names}
        self.buf = to_device(host, dtype)
        assert self.buf.data_ptr() % 16 == 0
        self.t = {k: self.buf[at[k]:at[k] + self.sizes[k]] for k in names}
        torch.cuda.synchronize()

    def ptr(self, k):
        return self.t[k].data_ptr()

    def get(self, k, shape):
        from nsol_amd.device import to_numpy
        return to_numpy(self.t[k], self.dtype).astype(np.float64).reshape(shape)

    def guards_intact(self):
        from nsol_amd.device import to_numpy
        host = to_numpy(self.buf, self.dtype)
        return bool(np.all(host[self.mask] == self.dtype(SENTINEL)))
