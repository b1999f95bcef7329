"""Guard bands and poison fills for device memory the kernels are handed (tests/test_gpu_workspace_hygiene.py, tests/test_gpu_op_guards.py;
tests/test_workspace_guard_helper.py checks this module on CPU tensors).

Every other GPU test compares values.  These helpers ask the two questions a value cannot answer: WHERE did a kernel write, and does a result
depend on bytes that are no operand of it?

    banded(nbytes, device)      one uint8 allocation [band | interior | band]: the interior starts `align`-aligned (what the arena and torch
                                give), the trailing band at the very first byte behind it (no rounding); .check() names the first changed
                                band byte
    flush(t, band_byte)         a copy of t whose last element is followed by band at once: a read past an operand's end that reaches a
                                result shows as a dependence on band_byte
    install(engine, batch, b)   the engine's workspace as a banded allocation of EXACTLY capf_workspace_bytes(batch), filled with b;
                                .refill(b) fills again and hands it over again (capf_set_workspace: everything the engine kept is gone)
    guarded_allocations()       for its duration torch.empty returns interiors of banded allocations pre-filled with 0xFF, all bands
                                checked on exit (capf/lib.py looks torch.empty up at call time: every stand-alone wrapper's outputs)

The fill bytes: 0x00 is 0 in every format; 0xFF is NaN in fp32, bf16 and fp16 and -1 as int32; 0x7F is 3.39e38 (finite) in fp32 and bf16,
NaN in fp16, 2139062143 as int32.  The band size is a condition, not a measurement: 4 MiB on each side."""
import contextlib
import ctypes

import torch

BAND = 4 << 20
BAND_BYTE = 0xA5
FILLS = (0x00, 0xFF, 0x7F)

_real_empty = torch.empty


class BandError(AssertionError):
    pass


class Banded:
    def __init__(self, nbytes, device, band=BAND, band_byte=BAND_BYTE, align=256):
        self.nbytes, self.band, self.band_byte = int(nbytes), int(band), int(band_byte)
        self.raw = _real_empty(self.band + align + self.nbytes + self.band, dtype=torch.uint8, device=device)
        start = self.band + (-(self.raw.data_ptr() + self.band)) % align
        self.raw.fill_(self.band_byte)
        self.head = self.raw[start - self.band:start]
        self.interior = self.raw[start:start + self.nbytes]
        self.tail = self.raw[start + self.nbytes:start + self.nbytes + self.band]

    def fill(self, byte):
        self.interior.fill_(int(byte))
        return self

    def check(self, what="allocation"):
        """Synchronise, then raise BandError naming the first changed band byte: >= 0 counts from the first byte behind the interior,
        < 0 back from the interior's first byte (-1 is the byte right in front of it)."""
        if self.raw.is_cuda:
            torch.cuda.synchronize(self.raw.device)
        for name, part, origin in (("trailing", self.tail, 0), ("leading", self.head, -self.band)):
            bad = part != self.band_byte
            if bool(bad.any()):
                first = int(torch.nonzero(bad)[0, 0])
                n = int(bad.sum())
                raise BandError(f"{what}: {name} band changed at offset {first + origin} from the interior's {'end' if origin == 0 else 'start'} "
                                f"(interior of {self.nbytes} bytes; byte now 0x{int(part[first]):02X}, band 0x{self.band_byte:02X}; {n} band bytes changed)")


def banded(nbytes, device, band=BAND, band_byte=BAND_BYTE, align=256):
    return Banded(nbytes, device, band, band_byte, align)


def _typed(b, shape, dtype):
    t = b.interior.view(dtype).view(shape) if b.nbytes else _real_empty(shape, dtype=dtype, device=b.raw.device)
    t._guard = b
    return t


def flush(t, band_byte, band=BAND):
    """A contiguous copy of t inside a banded allocation: its first element aligned, the first byte behind its last element band."""
    b = Banded(t.numel() * t.element_size(), t.device, band=band, band_byte=band_byte)
    c = _typed(b, t.shape, t.dtype)
    c.copy_(t)
    return c


def filled(shape, dtype, device, fill_byte, band=BAND):
    """An output tensor in a banded allocation (band BAND_BYTE) whose every byte is fill_byte."""
    n = 1
    for v in shape:
        n *= int(v)
    b = Banded(n * _real_empty(0, dtype=dtype).element_size(), device, band=band).fill(fill_byte)
    return _typed(b, tuple(shape), dtype)


def guard_of(t):
    return t._guard


def check_all(tensors, what="tensor"):
    for i, t in enumerate(tensors):
        guard_of(t).check(f"{what}[{i}]")


class Workspace:
    def __init__(self, engine, batch, fill_byte, band=BAND):
        self.engine, self.batch = engine, batch
        self.nbytes = engine.workspace_bytes(batch)
        assert self.nbytes > 0 and self.nbytes % 4 == 0, self.nbytes
        self.mem = Banded(self.nbytes, f"cuda:{engine.device}", band=band)
        engine._ws = self.mem.interior.view(torch.float32)
        engine._ws_batch = batch
        self.refill(fill_byte)

    def refill(self, fill_byte):
        self.mem.fill(fill_byte)
        e = self.engine
        e._check(e.lib.capf_set_workspace(e.h, ctypes.c_void_p(self.mem.interior.data_ptr()), self.nbytes), "set_workspace")
        return self

    def check(self, what="workspace"):
        self.mem.check(what)


def install(engine, batch, fill_byte, band=BAND):
    """Point `engine` at a banded workspace of exactly engine.workspace_bytes(batch) bytes (no slack), every byte fill_byte."""
    return Workspace(engine, batch, fill_byte, band)


@contextlib.contextmanager
def guarded_allocations(fill_byte=0xFF, band=BAND):
    """torch.empty -> the interior of a banded allocation pre-filled with fill_byte; every band is checked on the way out (also when the
    body raised: the body's exception wins).  Yields the list of Banded objects handed out so far."""
    made = []

    def empty(*args, **kwargs):
        if kwargs.get("out") is not None:
            return _real_empty(*args, **kwargs)
        probe = _real_empty(*args, **{**kwargs, "device": "meta"})
        device = kwargs.get("device")
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        b = Banded(probe.numel() * probe.element_size(), device, band=band).fill(fill_byte)
        made.append(b)
        t = _typed(b, probe.shape, probe.dtype)
        if kwargs.get("requires_grad"):
            t.requires_grad_(True)
        return t

    saved = torch.empty
    torch.empty = empty
    try:
        yield made
    except BaseException:
        torch.empty = saved
        raise
    else:
        torch.empty = saved
        for i, b in enumerate(made):
            b.check(f"torch.empty #{i} ({b.nbytes} bytes)")
    finally:
        torch.empty = saved
