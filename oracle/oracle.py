"""ctypes bindings for the CHECKERS under oracle/ -- test infrastructure only.

Only tests/, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import
this module.  The product (``nblic-image-compression_amd``) never does.

Two libraries:

* ``liboracle.so``            our CPU restatement (``Oracle``), always available after ``make``;
* ``_ref/libnblic_ref.so``    the unmodified reference compiled in this container
                              (``Reference``), present only when it was built here or shipped
                              as a prebuilt file; nothing reads /root/reference at run time.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_u8p = C.POINTER(C.c_uint8)


def _ptr(a: np.ndarray, ty=_u8p):
    return a.ctypes.data_as(ty)


def build(force: bool = False) -> None:
    """Compile liboracle.so (and oracle/_ref when /root/reference is present)."""
    so = os.path.join(_HERE, "liboracle.so")
    srcs = [os.path.join(_HERE, f) for f in os.listdir(_HERE) if f.endswith((".c", ".h"))]
    stale = force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if stale:
        subprocess.run(["make", "-C", _HERE, "liboracle.so"], check=True, capture_output=True)
    if os.path.isdir("/root/reference/src"):
        for target, name in (("ref", "libnblic_ref.so"), ("ref_big", "libnblic_ref_big.so"),       # ref_big: config 5's raised pixel limit
                             ("ref_fileio", "libfileio_ref.so"), ("ref_main", "NBLIC_main.o")):       # the front end's checks
            if force or not os.path.exists(os.path.join(_HERE, "_ref", name)):
                subprocess.run(["make", "-C", _HERE, target], check=True, capture_output=True)


def syn1(h: int, w: int, seed: int = 1) -> np.ndarray:
    """SYN-1 deterministic frame, via the C generator."""
    img = np.empty((h, w), np.uint8)
    Oracle().lib.orc_syn1(_ptr(img), h, w, C.c_uint32(seed))
    return img


def out_capacity(h: int, w: int) -> int:
    return 2 * h * w + 4096


class Oracle:
    """Our restatement: fused engine + staged -e1 pipeline + QNBLIC."""

    _lib = None

    def __init__(self):
        if Oracle._lib is None:
            build()
            lib = C.CDLL(os.path.join(_HERE, "liboracle.so"))
            lib.orc_nblic_encode.restype = C.c_long
            lib.orc_nblic_encode.argtypes = [_u8p, _u8p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_long, C.POINTER(C.c_long)]
            lib.orc_nblic_encode_kstep.restype = C.c_long
            lib.orc_nblic_encode_kstep.argtypes = [_u8p, _u8p] + [C.c_int] * 5
            lib.orc_walk_coverage.restype = None
            lib.orc_walk_coverage.argtypes = [C.POINTER(C.c_long)]
            lib.orc_nblic_decode.restype = C.c_int
            lib.orc_nblic_decode.argtypes = [_u8p, _u8p] + [C.POINTER(C.c_int)] * 4 + [C.c_long]
            lib.orc_nblic_encode_staged.restype = C.c_long
            lib.orc_nblic_encode_staged.argtypes = [_u8p, _u8p, C.c_int, C.c_int, C.POINTER(C.c_long)]
            lib.orc_syn1.restype = None
            lib.orc_syn1.argtypes = [_u8p, C.c_int, C.c_int, C.c_uint32]
            for name in ("orc_qnblic_encode", "orc_qnblic_decode"):
                if hasattr(lib, name):
                    getattr(lib, name).restype = C.c_long
            Oracle._lib = lib
        self.lib = Oracle._lib

    # -- fused engine -----------------------------------------------------
    def encode(self, img: np.ndarray, near: int = 0, effort: int = 1, max_px: int = 0, k_step=None):
        """Returns (stream bytes, reconstruction, near_out, effort_out, n_bins).  k_step=None: the encoders' own
        clip(3 + 2 near, 3, 16).  A k_step given goes into the header as it is (orc_nblic_encode_kstep): nothing is
        clamped, arguments a decoder would refuse give a None stream, and n_bins is not counted (0)."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        rec = img.copy()
        out = np.empty(out_capacity(h, w), np.uint8)
        if k_step is not None:
            ln = self.lib.orc_nblic_encode_kstep(_ptr(out), _ptr(rec), h, w, int(near), int(k_step), int(effort))
            return (None if ln < 0 else out[:ln].tobytes()), rec, int(near), int(effort), 0
        n, e, nb = C.c_int(near), C.c_int(effort), C.c_long(0)
        ln = self.lib.orc_nblic_encode(_ptr(out), _ptr(rec), h, w, C.byref(n), C.byref(e), max_px, C.byref(nb))
        if ln < 0:
            return None, rec, n.value, e.value, 0
        return out[:ln].tobytes(), rec, n.value, e.value, nb.value

    def walk_coverage(self) -> dict:
        """Which parts of the binarisation walk the last ``encode`` visited (the oracle's own counters; the product has
        none): symbols per starting level ``qu`` (16) and per suffix length ``k``, ``escalations`` to the next level's
        tree, and ``beyond_lanes``, symbols whose prefix has at least min(256 >> k_max, 64) ones."""
        v = (C.c_long * 26)()
        self.lib.orc_walk_coverage(v)
        return {"qu": list(v[:16]), "k": list(v[16:24]), "escalations": int(v[24]), "beyond_lanes": int(v[25])}

    def decode(self, stream: bytes, max_px: int = 0):
        """Returns (image, near, effort) or None."""
        buf = np.frombuffer(bytes(stream) + b"\0" * 16, np.uint8).copy()
        if len(stream) < 16:
            return None
        h = (int(buf[9]) << 8) | int(buf[10])
        w = (int(buf[11]) << 8) | int(buf[12])
        img = np.zeros((max(h, 1), max(w, 1)), np.uint8)
        hh, ww, n, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        rc = self.lib.orc_nblic_decode(_ptr(buf), _ptr(img), C.byref(hh), C.byref(ww), C.byref(n), C.byref(e), max_px)
        if rc != 0:
            return None
        return img, n.value, e.value

    # -- staged -e1 lossless ----------------------------------------------
    def encode_staged(self, img: np.ndarray):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.empty(out_capacity(h, w), np.uint8)
        ne = C.c_long(0)
        ln = self.lib.orc_nblic_encode_staged(_ptr(out), _ptr(img), h, w, C.byref(ne))
        return out[:ln].tobytes(), ne.value

    def stages(self, img: np.ndarray) -> dict:
        """Every intermediate array of the staged -e1 lossless pipeline (for kernel parity)."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        n = h * w
        L = self.lib
        u16p = C.POINTER(C.c_uint16)
        px0 = np.empty(n, np.uint8); err = np.empty(n, np.int8)
        qu = np.empty(n, np.uint8); qv = np.empty(n, np.uint8); qw = np.empty(n, np.uint8)
        adr = np.empty(n, np.uint16)
        L.orc_s1(_ptr(img), h, w, _ptr(px0), err.ctypes.data_as(C.POINTER(C.c_int8)), _ptr(qu), _ptr(qv), _ptr(qw), _ptr(adr, u16p))
        px = np.empty(n, np.uint8); sign = np.empty(n, np.uint8)
        L.orc_s2(C.c_size_t(n), _ptr(adr, u16p), _ptr(px0), err.ctypes.data_as(C.POINTER(C.c_int8)), _ptr(px), _ptr(sign))
        y = np.empty(n, np.uint8); z = np.empty(n, np.uint8)
        L.orc_s3(C.c_size_t(n), _ptr(img), _ptr(px), _ptr(sign), _ptr(y), _ptr(z))
        L.orc_s4.restype = C.c_size_t
        cnt = np.empty(n, np.uint8)
        ne = L.orc_s4(C.c_size_t(n), _ptr(qu), _ptr(qv), _ptr(qw), _ptr(z), None, None, None, None, None)
        cu = np.empty(ne, np.uint16); cv = np.empty(ne, np.uint16)
        eqw = np.empty(ne, np.uint8); ebin = np.empty(ne, np.uint8)
        L.orc_s4(C.c_size_t(n), _ptr(qu), _ptr(qv), _ptr(qw), _ptr(z), _ptr(cu, u16p), _ptr(cv, u16p), _ptr(eqw), _ptr(ebin), _ptr(cnt))
        prob = np.empty(ne, np.uint16)
        L.orc_s5(C.c_size_t(ne), _ptr(cu, u16p), _ptr(cv, u16p), _ptr(eqw), _ptr(ebin), _ptr(prob, u16p))
        out = np.empty(out_capacity(h, w), np.uint8)
        L.orc_s6.restype = C.c_size_t
        nbody = L.orc_s6(C.c_size_t(ne), _ptr(prob, u16p), _ptr(ebin), _ptr(out))
        return dict(px0=px0, err=err, qu=qu, qv=qv, qw=qw, adr=adr, px=px, sign=sign, y=y, z=z,
                    ev_count=cnt, cu=cu, cv=cv, ev_qw=eqw, ev_bin=ebin, prob=prob, body=out[:nbody].tobytes())

    # -- the staged entropy front of every mode ---------------------------
    def trace(self, img: np.ndarray, near: int = 0, effort: int = 1) -> dict:
        """The fused encoder of (near, effort), k_step paired with near (orc_nblic_trace): ``stream``, ``recon`` and, per
        pixel in raster order, what the model stage hands to the entropy front (``px0``, ``adr``, ``qu``, ``qv``,
        ``qw``, ``px``, ``sign``) and what the front makes of it (``y``, ``z``, ``bins``)."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        rec = img.copy()
        out = np.empty(out_capacity(h, w), np.uint8)
        names = ("px0", "adr", "qu", "qv", "qw", "px", "sign", "y", "z", "bins")
        t = {k: np.empty(h * w, np.uint16 if k == "adr" else np.uint8) for k in names}
        fn = self.lib.orc_nblic_trace
        fn.restype = C.c_long
        ln = fn(_ptr(out), _ptr(rec), h, w, int(near), int(effort), *[C.c_void_p(t[k].ctypes.data) for k in names])
        if ln < 0:
            raise ValueError("orc_nblic_trace refused its arguments")
        t.update(stream=out[:ln].tobytes(), recon=rec)
        return t

    def s3_near(self, x, px, sign, near: int):
        """orc_s3_near on flat arrays: (y, z)."""
        x, px, sign = (np.ascontiguousarray(a, np.uint8).reshape(-1) for a in (x, px, sign))
        y, z = np.empty(x.size, np.uint8), np.empty(x.size, np.uint8)
        self.lib.orc_s3_near(C.c_size_t(x.size), _ptr(x), _ptr(px), _ptr(sign), int(near), _ptr(y), _ptr(z))
        return y, z

    def s4_kstep(self, k_step: int, qu, qv, qw, z) -> dict:
        """orc_s4_kstep on flat arrays: ``cnt`` (bins per record) and the events ``cu``, ``cv``, ``qw``, ``bin``."""
        qu, qv, qw, z = (np.ascontiguousarray(a, np.uint8).reshape(-1) for a in (qu, qv, qw, z))
        n = qu.size
        u16p = C.POINTER(C.c_uint16)
        fn = self.lib.orc_s4_kstep
        fn.restype = C.c_size_t
        ne = fn(C.c_size_t(n), int(k_step), _ptr(qu), _ptr(qv), _ptr(qw), _ptr(z), None, None, None, None, None)
        cu, cv = np.empty(ne, np.uint16), np.empty(ne, np.uint16)
        eqw, ebin, cnt = np.empty(ne, np.uint8), np.empty(ne, np.uint8), np.empty(n, np.uint8)
        fn(C.c_size_t(n), int(k_step), _ptr(qu), _ptr(qv), _ptr(qw), _ptr(z), _ptr(cu, u16p), _ptr(cv, u16p), _ptr(eqw), _ptr(ebin), _ptr(cnt))
        return dict(cnt=cnt, cu=cu, cv=cv, qw=eqw, bin=ebin)

    def s5(self, cu, cv, qw, bin_) -> np.ndarray:
        """orc_s5: the probability of every event."""
        cu, cv = np.ascontiguousarray(cu, np.uint16), np.ascontiguousarray(cv, np.uint16)
        qw, bin_ = np.ascontiguousarray(qw, np.uint8), np.ascontiguousarray(bin_, np.uint8)
        u16p = C.POINTER(C.c_uint16)
        prob = np.empty(cu.size, np.uint16)
        self.lib.orc_s5(C.c_size_t(cu.size), _ptr(cu, u16p), _ptr(cv, u16p), _ptr(qw), _ptr(bin_), _ptr(prob, u16p))
        return prob

    def s6(self, prob, bin_) -> bytes:
        """orc_s6: the range coder's bytes (flush included, no header)."""
        prob, bin_ = np.ascontiguousarray(prob, np.uint16), np.ascontiguousarray(bin_, np.uint8)
        out = np.empty(2 * prob.size + 64, np.uint8)
        self.lib.orc_s6.restype = C.c_size_t
        n = self.lib.orc_s6(C.c_size_t(prob.size), _ptr(prob, C.POINTER(C.c_uint16)), _ptr(bin_), _ptr(out))
        return out[:n].tobytes()

    # -- QNBLIC (effort 0) ------------------------------------------------
    def qencode(self, img: np.ndarray):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.empty(out_capacity(h, w) // 2, np.uint16)
        words = self.lib.orc_qnblic_encode(out.ctypes.data_as(C.POINTER(C.c_uint16)), _ptr(img), h, w, C.c_long(0))
        return None if words < 0 else out[:words].tobytes()

    def qdecode(self, stream: bytes):
        buf = np.frombuffer(bytes(stream) + b"\0" * 16, np.uint8).copy().view(np.uint16)
        if len(stream) < 8:
            return None
        h, w = int(buf[2]), int(buf[3])
        img = np.zeros((max(h, 1), max(w, 1)), np.uint8)
        hh, ww = C.c_int(), C.c_int()
        rc = self.lib.orc_qnblic_decode(buf.ctypes.data_as(C.POINTER(C.c_uint16)), _ptr(img), C.byref(hh), C.byref(ww), C.c_long(0))
        return None if rc != 0 else img

    def q_model(self, img: np.ndarray):
        """orc_q_model: per pixel in raster order the level ``qd`` and the symbol ``y`` the entropy stage codes, and the
        12 x 256 counts ``hist`` of the symbols per level.  Returns (qd, y, hist)."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        qd, y = np.empty(h * w, np.uint8), np.empty(h * w, np.uint8)
        hist = np.zeros((12, 256), np.uint32)
        self.lib.orc_q_model.restype = None
        self.lib.orc_q_model(_ptr(img), h, w, None, None, _ptr(qd), _ptr(y), C.c_void_p(hist.ctypes.data))
        return qd, y, hist

    def q_norm_hist(self, hist) -> np.ndarray:
        """orc_q_norm_hist on one 256-entry histogram: its scaling to a sum of 2^15 (a copy; the argument is left alone)."""
        out = np.ascontiguousarray(hist, np.uint32).reshape(256).copy()
        self.lib.orc_q_norm_hist.restype = None
        self.lib.orc_q_norm_hist(C.c_void_p(out.ctypes.data))
        return out

    def qencode_tables(self, img: np.ndarray, tables, model=None) -> bytes:
        """The QNBLIC stream of ``img`` coded with the caller's 12 x 256 ``tables`` in place of the image's own counts
        (orc_q_entropy_stage with hist_in = tables).  The stage scales what it is given (orc_q_norm_hist), so the stream
        carries ``tables`` themselves only where every level is a fixed point of that scaling; every symbol the image
        codes needs a nonzero entry (ValueError otherwise: the coder would divide by zero).  ``model``: the
        ``q_model(img)`` triple when the caller has it already."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        qd, y, _ = self.q_model(img) if model is None else model
        tables = np.ascontiguousarray(tables, np.uint32).reshape(12, 256)
        if (tables[qd, y] == 0).any():
            raise ValueError("a coded symbol has no entry in the tables")
        out = np.empty(h * w + 4 + 12 * 256 + 2, np.uint16)              # header, 12 x 256 codes, a word per pixel, the state
        fn = self.lib.orc_q_entropy_stage
        fn.restype = C.c_long
        words = fn(C.c_void_p(out.ctypes.data), h, w, _ptr(qd), _ptr(y), C.c_void_p(tables.ctypes.data))
        assert 0 < words <= out.size
        return out[:words].tobytes()


class Reference:
    """The unmodified reference library compiled into oracle/_ref (never shipped in git)."""

    path = os.path.join(_HERE, "_ref", "libnblic_ref.so")

    @classmethod
    def available(cls) -> bool:
        return os.path.exists(cls.path)

    def __init__(self):
        lib = C.CDLL(self.path)
        lib.NBLICcompress.restype = C.c_int
        lib.NBLICcompress.argtypes = [C.c_int, _u8p, _u8p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.NBLICdecompress.restype = C.c_int
        lib.NBLICdecompress.argtypes = [C.c_int, _u8p, _u8p] + [C.POINTER(C.c_int)] * 4
        u16p = C.POINTER(C.c_uint16)
        lib.QNBLICcompress.restype = C.c_int
        lib.QNBLICcompress.argtypes = [u16p, _u8p, C.c_int, C.c_int]
        lib.QNBLICdecompress.restype = C.c_int
        lib.QNBLICdecompress.argtypes = [u16p, _u8p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.lib = lib

    def encode(self, img: np.ndarray, near: int = 0, effort: int = 1):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        rec = img.copy()
        out = np.empty(out_capacity(h, w), np.uint8)
        n, e = C.c_int(near), C.c_int(effort)
        ln = self.lib.NBLICcompress(0, _ptr(out), _ptr(rec), h, w, C.byref(n), C.byref(e))
        if ln < 0:
            return None, rec, n.value, e.value
        return out[:ln].tobytes(), rec, n.value, e.value

    def decode(self, stream: bytes):
        buf = np.frombuffer(bytes(stream) + b"\0" * 16, np.uint8).copy()
        h = (int(buf[9]) << 8) | int(buf[10])
        w = (int(buf[11]) << 8) | int(buf[12])
        img = np.zeros((max(h, 1), max(w, 1)), np.uint8)
        hh, ww, n, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        rc = self.lib.NBLICdecompress(0, _ptr(buf), _ptr(img), C.byref(hh), C.byref(ww), C.byref(n), C.byref(e))
        return None if rc != 0 else (img, n.value, e.value)

    def qencode(self, img: np.ndarray):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.empty(out_capacity(h, w) // 2, np.uint16)
        words = self.lib.QNBLICcompress(out.ctypes.data_as(C.POINTER(C.c_uint16)), _ptr(img), h, w)
        return None if words < 0 else out[:words].tobytes()

    def qdecode(self, stream: bytes):
        buf = np.frombuffer(bytes(stream) + b"\0" * 16, np.uint8).copy().view(np.uint16)
        h, w = int(buf[2]), int(buf[3])
        img = np.zeros((max(h, 1), max(w, 1)), np.uint8)
        hh, ww = C.c_int(), C.c_int()
        rc = self.lib.QNBLICdecompress(buf.ctypes.data_as(C.POINTER(C.c_uint16)), _ptr(img), C.byref(hh), C.byref(ww))
        return None if rc != 0 else img
