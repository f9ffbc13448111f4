"""What the block filters share, and the chain a receiver runs its blocks through.

``BlockFilter`` is the wrapper of a handle that turns blocks of cfg.ngps samples (complex64, or the
recorder's uint16) into complex64 blocks of the same length: ``excision.Excision`` (gpsmi_ifx_*),
``tfexcision.SweepExcision`` (gpsmi_tfx_*) and ``blanking.PulseBlanker`` (gpsmi_pb_*) are subclasses,
and ``nulling.NullSteer`` (gpsmi_nul_*), whose input is the blocks of several antennas.
``Conditioner`` is the chain recording -> (null steering) -> (excision) -> (sweep excision) ->
(blanking) -> the complex64 block the engines see, one block per call.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from .engine import Config, DeviceBuffer, PinnedArray


class BlockFilter:
    """A subclass names its functions (PREFIX: gpsmi_<PREFIX>_* of gpsmi.h), makes the cfg struct
    for _create in its constructor and the result arrays of a call in _results."""
    PREFIX = None

    def __init__(self, cfg, raw_u8):
        self.cfg = cfg or Config()
        self.lib = _lib.load()
        self.n = self.cfg.ngps
        self.raw_u8 = bool(raw_u8)
        self.last_nb = 0                # blocks of the last call that ran

    def _call(self, name, *args):
        name = f'gpsmi_{self.PREFIX}_{name}'
        check(getattr(self.lib, name)(*args), name)

    def _create(self, c):
        h = C.c_void_p()
        self._call('create', C.byref(c), C.byref(h))
        self.h = h
        if self.raw_u8:
            self._call('set_input_format', self.h, 1)

    def _results(self, nb):
        """Fresh last_* arrays for nb blocks -> them, in the order the ABI takes them."""
        raise NotImplementedError

    def apply(self, blocks, out=None):
        """Host blocks in (one block [n] or consecutive blocks [nb, n]; complex64, or uint16 with
        raw_u8), complex64 of the same shape out (into `out` when given, e.g. page-locked memory)."""
        want = np.uint16 if self.raw_u8 else np.complex64
        x = np.asarray(blocks)
        if x.dtype != want:
            raise TypeError(f'blocks dtype {x.dtype} does not match the input format '
                            f'({np.dtype(want).name})')
        if x.size == 0 or x.size % self.n:
            raise ValueError(f'blocks of {self.n} samples expected, got {x.shape}')
        x = np.ascontiguousarray(x)
        nb = x.size // self.n
        if out is None:
            out = np.empty(x.shape, dtype=np.complex64)
        elif out.dtype != np.complex64 or out.size != x.size or not out.flags['C_CONTIGUOUS']:
            raise ValueError('out must be a C-contiguous complex64 array of the input size')
        self._call('apply', self.h, ptr(x), ptr(out), nb, *map(ptr, self._results(nb)))
        self.last_nb = nb
        return out

    def apply_dev(self, d_in, d_out, nb):
        """nb consecutive blocks from device memory (c_void_p or int) to device memory (complex64)."""
        self._call('apply_dev', self.h, d_in, d_out, int(nb), *map(ptr, self._results(int(nb))))
        self.last_nb = int(nb)

    def reset(self):
        """Carry := 0, as after creation (nothing of the block before reaches the next one)."""
        self._call('reset', self.h)

    def last_ms(self):
        ms = C.c_float(0.0)
        self._call('last_ms', self.h, C.byref(ms))
        return ms.value

    def close(self):
        if getattr(self, 'h', None):
            self._call('destroy', self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _wanted(arg):
    return arg is not None and arg is not False


class Conditioner:
    """excise / blank / null / sweep: True (a stage of default settings, made and closed here), an
    Excision / a PulseBlanker / a NullSteer / a SweepExcision of the caller's (used, not closed), or
    None / False (off); sweep may also be a frame length (32 .. 256) for a stage made here.  raw_u8:
    apply() takes the recorder's uint16 blocks; with any stage on it returns complex64 (out_raw_u8
    False).  The order is null steering, excision, sweep excision, blanking, and only the first stage
    takes the raw format (the others: raw_u8=False).  Null steering goes first: it needs every antenna,
    and what it leaves is one complex64 block like any other; with it apply() takes [antennas][n].  A
    tone raises every sample's power and would hide the pulses from the blanker, while the pulses only
    add a flat level to the excision's spectrum: excision before blanking.  A constant-envelope sweep
    does the same to the blanker's median and also only adds a flat level to the tone excision's
    spectrum: the sweep excision stands between the two.  A chain without a stage is falsy and passes
    every block through."""

    def __init__(self, cfg, raw_u8, excise=None, blank=None, null=None, antennas=1, sweep=None):
        self.cfg, self.raw_u8 = cfg, bool(raw_u8)
        self.antennas = int(antennas)
        self.nuller = self.excision = self.sweeper = self.blanker = self.last = None
        self._owned, self._pinned, self._dev = [], None, []
        if _wanted(null):
            from .nulling import NullSteer
            if self.antennas < 2:
                raise ValueError('null steering needs antennas >= 2')
            self.nuller = self._stage(NullSteer, null, self.raw_u8, antennas=self.antennas)
            if self.nuller.antennas != self.antennas:
                raise ValueError('the NullSteer does not match the number of antennas')
        elif self.antennas != 1:
            raise ValueError('several antennas need null=...: nothing else combines them')
        if _wanted(excise):
            from .excision import Excision
            self.excision = self._stage(Excision, excise, self.raw_u8 and self.nuller is None)
        if _wanted(sweep):
            from .tfexcision import SweepExcision      # (behind the stages before it: their complex64)
            kw = {}
            if isinstance(sweep, int) and not isinstance(sweep, bool):      # (a frame length: made here)
                kw, sweep = dict(frame=sweep), True
            self.sweeper = self._stage(SweepExcision, sweep,
                                       self.raw_u8 and self.nuller is None and self.excision is None, **kw)
        if _wanted(blank):
            from .blanking import PulseBlanker
            self.blanker = self._stage(PulseBlanker, blank, self.raw_u8 and self.nuller is None and
                                       self.excision is None and self.sweeper is None)
        self.stages = [s for s in (self.nuller, self.excision, self.sweeper, self.blanker) if s is not None]
        self.out_raw_u8 = self.raw_u8 and not self.stages
        n = cfg.ngps
        if self.stages:
            self._pinned = PinnedArray((n,), np.complex64)
        if len(self.stages) > 1:                        # the input, then one block behind every stage
            sizes = [n * self.antennas * (2 if self.raw_u8 else 8)] + [n * 8] * len(self.stages)
            self._dev = [DeviceBuffer(b, cfg.device) for b in sizes]

    def _stage(self, cls, arg, raw_u8, **kw):
        stage = arg
        if arg is True:
            stage = cls(self.cfg, raw_u8=raw_u8, **kw)
            self._owned.append(stage)
        if stage.raw_u8 != raw_u8 or stage.n != self.cfg.ngps:
            raise ValueError(f'the {cls.__name__} does not match raw_u8 / the block length')
        return stage

    def __bool__(self):
        return bool(self.stages)

    def apply(self, block):
        """One block ([antennas][n] with null steering) -> the block the engines see: `block` itself
        without a stage, else the chain's one page-locked complex64 block (use it, or copy it, before
        the next call)."""
        if len(self.stages) == 1:
            block = self.stages[0].apply(block, out=self._pinned.array)
        elif self.stages:                               # one copy in, every stage on the device, one out
            want = np.uint16 if self.raw_u8 else np.complex64
            x = np.ascontiguousarray(block)
            if x.dtype != want or x.size != self.cfg.ngps * self.antennas:
                raise ValueError(f'one block of {self.cfg.ngps} {np.dtype(want).name} samples '
                                 f'(of each of {self.antennas} antennas) expected')
            self._dev[0].upload(x)
            for stage, d_in, d_out in zip(self.stages, self._dev, self._dev[1:]):
                stage.apply_dev(d_in.ptr, d_out.ptr, 1)
            block = self._dev[-1].download_into(self._pinned.array)
        self.last = block
        return block

    def close(self):
        self.last = None
        if self._pinned is not None:
            self._pinned.free()
            self._pinned = None
        for x in self._dev:
            x.free()
        for s in self._owned:
            s.close()
        self._dev, self._owned = [], []
