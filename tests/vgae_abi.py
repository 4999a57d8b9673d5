"""Device-side plumbing shared by tests/test_gpu_noise.py and tests/test_gpu_vgae_head.py: outputs with canaries, a
dense_ref.Arena copied to the GPU, the draw counter as a device word, and one gae_x_vgae_head_prep call with every byte
of the loss workspace it may and may not write accounted for."""
import ctypes

import numpy as np
import torch

import dense_ref

DEV = "cuda:0"
CANARY = 0x7FC0BEEF                       # dense_ref.PATTERN: a quiet NaN no kernel here produces
SEED = 0x9E3779B97F4A7C15                 # both halves non-zero
M64 = (1 << 64) - 1


def lib():
    from gae_dgl_amd import _lib
    return _lib.load()


def stream():
    from gae_dgl_amd.ops import _stream
    return _stream()


def draw_tensor(draw):
    """the device word gae_* read as *draw_dev (None: a NULL pointer = draw 0)"""
    if draw is None:
        return None
    draw = int(draw) & M64
    return torch.tensor([draw - (1 << 64) if draw >= (1 << 63) else draw], dtype=torch.int64, device=DEV)


def ptr(t, offset_bytes=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset_bytes)


class Canaried:
    """an output of n 32-bit words with 64 canary words in front of it and 64 behind it"""

    def __init__(self, n):
        self.n = int(n)
        self.whole = torch.full((self.n + 128,), CANARY, dtype=torch.int32, device=DEV)
        assert self.whole.data_ptr() % 16 == 0

    def ptr(self):
        return ctypes.c_void_p(self.whole.data_ptr() + 256)

    def bits(self):
        torch.cuda.synchronize()
        return self.whole.cpu().numpy().view(np.uint32)

    def read(self):
        """(values fp32 [n], canaries intact)"""
        b = self.bits()
        return b[64:64 + self.n].view(np.float32).copy(), bool((b[:64] == CANARY).all() and (b[64 + self.n:] == CANARY).all())


class Device:
    """a dense_ref.Arena and its copy on the GPU"""

    def __init__(self, arena):
        self.a = arena
        self.dev = torch.from_numpy(arena.host.view(np.int32).copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.before = arena.host.copy()

    def ptr(self, name, offset_floats=0):
        return ctypes.c_void_p(self.dev.data_ptr() + 4 * (self.a.offset(name) + offset_floats))

    def download(self):
        torch.cuda.synchronize()
        self.a.host = self.dev.cpu().numpy().view(np.uint32).copy()

    def f64(self, name):
        """a workspace operand read as doubles"""
        return self.a.bits(name).reshape(-1).view(np.float64)

    def check_memory(self, what, inputs, outputs):
        """guards intact, inputs bit-unchanged with their pads, output pads still the pattern, no NaN in an output"""
        a = self.a
        assert a.guards_intact() and all(a.pads_intact(k) for k in a.ops), \
            (what, "written outside an operand (word, nearest operand, offset from its base):", a.damaged())
        for name in inputs:
            o = a.ops[name]
            assert np.array_equal(a.footprint(name), self.before[o["base"]:o["base"] + o["rows"] * o["ld"]]), \
                (what, f"input {name} changed")
        for name in outputs:
            assert a.pads_intact(name), (what, f"pad columns of {name} written")
            got = a.get(name)
            assert not np.isnan(got).any(), (what, f"NaN in {name}", np.argwhere(np.isnan(got))[:4].tolist())


class PrepWorkspace:
    """the loss workspace of gae_decoder_bce for (n, 16), filled with a byte pattern, and its gae_bce_prep layout"""
    FILL = 0xA5

    def __init__(self, n):
        from gae_dgl_amd import _lib
        L = lib()
        self.n, self.blocks = n, (n + 63) // 64
        self.bytes = int(L.gae_decoder_bce_workspace_bytes(n, n, 16))
        assert self.bytes > 0
        self.ws = torch.full((self.bytes,), self.FILL, dtype=torch.uint8, device=DEV)
        self.lay = _lib.BcePrep()
        rc = L.gae_x_decoder_bce_prep_layout(n, 16, ptr(self.ws), self.bytes, ctypes.byref(self.lay))
        assert rc == 0, (rc, L.gae_last_error())
        assert self.lay.DP == 16 and self.lay.max_blocks >= self.blocks

    def _span(self, p, nbytes):
        o = int(p) - self.ws.data_ptr()
        assert 0 <= o and o + nbytes <= self.bytes
        return o, o + nbytes

    def read(self):
        """dict(Zt fp32 [n, 16], Zhi / Zlo uint16 [n, 16], colsum fp64 [blocks, 2, 16], clean): `clean` says that no
        byte outside those four pieces -- rows past n, blocks past ceil(n / 64), the rest of the workspace -- changed"""
        torch.cuda.synchronize()
        raw = self.ws.cpu().numpy()
        n, b = self.n, self.blocks
        spans = {"Zt": self._span(self.lay.Zt, n * 64), "Zhi": self._span(self.lay.Zhi, n * 32),
                 "Zlo": self._span(self.lay.Zlo, n * 32), "colsum": self._span(self.lay.colsum_partial, b * 256)}
        free = np.ones(self.bytes, bool)
        for lo, hi in spans.values():
            free[lo:hi] = False
        piece = {k: raw[lo:hi].copy() for k, (lo, hi) in spans.items()}
        return dict(Zt=piece["Zt"].view(np.float32).reshape(n, 16), Zhi=piece["Zhi"].view(np.uint16).reshape(n, 16),
                    Zlo=piece["Zlo"].view(np.uint16).reshape(n, 16), colsum=piece["colsum"].view(np.float64).reshape(b, 2, 16),
                    clean=bool((raw[free] == self.FILL).all()))


def arena():
    return dense_ref.Arena()
