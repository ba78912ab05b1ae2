"""The CPU specification of translucent blocks: tests/glass_port.c — oracle/port.c, included whole and untouched,
plus trace_sample_glass — built lazily into tests/libchunky_glass_port.so (git-ignored; it travels with the tree) with the flags of
oracle/Makefile's `port` rule, and wrapped in oracle.binding.PortLib, so that PortExt / PortOptions / PortCull apply to it as they do to
the oracle's own library.  A plain helper module: tests import it."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import binding

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libchunky_glass_port.so")
SOURCES = [os.path.join(HERE, "glass_port.c"), os.path.join(ROOT, "oracle", "port.c"), os.path.join(ROOT, "oracle", "oracle_scene.h"),
           os.path.join(ROOT, "chunkyclplugin_amd", "csrc", "glass_spec.h"), os.path.join(ROOT, "chunkyclplugin_amd", "csrc", "rt_math.h"),
           os.path.join(ROOT, "chunkyclplugin_amd", "csrc", "rt_pow_tables.inc")]
CENSUS_NAMES = ("main_crossings", "reflect_vertices", "sun_crossings", "emitter_crossings", "rm_skipped", "rm_resets", "capped", "tri_crossings",
                "rehits", "crossings")
DEFAULT = (0.99, 8)  # opaque_alpha, max_crossings


def _arch_flags():
    """oracle/Makefile's ARCH: -march=x86-64-v3 where the CPU has AVX2 and FMA."""
    try:
        flags = open("/proc/cpuinfo").read().split()
    except OSError:
        return []
    return ["-march=x86-64-v3"] if "avx2" in flags and "fma" in flags else []


def _build():
    # CHUNKY_ORACLE_NO_BUILD=1: never spawn a child (oracle/binding.py _make has the reason); the library must exist already
    if os.environ.get("CHUNKY_ORACLE_NO_BUILD"):
        return
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(s) for s in SOURCES):
        return
    cmd = [os.environ.get("CC", "gcc"), "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", *_arch_flags(), "-fopenmp", "-fPIC", "-shared",
           "-o", LIB + ".tmp", SOURCES[0], "-lm"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    os.replace(LIB + ".tmp", LIB)


class GlassLib(binding.PortLib):
    """PortLib over the glass library: every port_* call, and the glass entry points."""

    def __init__(self, path):
        super().__init__(path)
        L = self.lib
        L.glass_set.argtypes = [C.c_int, C.c_float, C.c_int]
        L.glass_set.restype = None
        L.glass_render_passes.argtypes = [C.POINTER(binding.OracleScene), C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int]
        L.glass_render_passes.restype = C.c_int
        L.glass_render_gids.argtypes = [C.POINTER(binding.OracleScene), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        L.glass_render_gids.restype = C.c_int
        L.glass_helpers.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.glass_helpers.restype = None
        L.glass_census_enable.argtypes = [C.c_int]
        L.glass_census_enable.restype = None
        L.glass_census_reset.restype = None
        L.glass_census_read.argtypes = [C.c_void_p]
        L.glass_census_read.restype = None
        assert L.glass_census_count() == len(CENSUS_NAMES)

    def glass_render_passes(self, sc, seeds, first_spp=0, res=None, gid_range=None, threads=8):
        h = sc if isinstance(sc, binding.SceneHandle) else binding.SceneHandle(sc)
        seeds = np.ascontiguousarray(seeds, np.int32)
        n = h.width * h.height
        if res is None:
            res = np.zeros(3 * n, np.float32)
        b, e = gid_range if gid_range is not None else (0, n)
        self.lib.glass_render_passes(C.byref(h.struct), seeds.ctypes.data, len(seeds), first_spp, b, e, res.ctypes.data, threads)
        return res

    def glass_render_gids(self, sc, seeds, gids, first_spp=0, res=None, threads=8):
        h = sc if isinstance(sc, binding.SceneHandle) else binding.SceneHandle(sc)
        seeds = np.ascontiguousarray(seeds, np.int32)
        gids = np.ascontiguousarray(gids, np.int32)
        if res is None:
            res = np.zeros(3 * h.width * h.height, np.float32)
        self.lib.glass_render_gids(C.byref(h.struct), seeds.ctypes.data, len(seeds), first_spp, gids.ctypes.data, gids.size, res.ctypes.data, threads)
        return res

    def helpers_glass(self, which, rows):
        """glass_helpers: rows of up to 12 floats in (padded with zeros), 4 floats out per row."""
        rows = np.asarray(rows, np.float32)
        rows = rows.reshape(len(rows), -1)
        full = np.zeros((len(rows), 12), np.float32)
        full[:, :rows.shape[1]] = rows
        out = np.zeros((len(rows), 4), np.float32)
        self.lib.glass_helpers(int(which), len(full), full.ctypes.data, out.ctypes.data)
        return out

    def census(self, enable=None, reset=False):
        if enable is not None:
            self.lib.glass_census_enable(1 if enable else 0)
        out = np.zeros(len(CENSUS_NAMES), np.int64)
        self.lib.glass_census_read(out.ctypes.data)
        if reset:
            self.lib.glass_census_reset()
        return dict(zip(CENSUS_NAMES, (int(v) for v in out)))


class Glass:
    """with Glass(lib, opaque_alpha, max_crossings): glass_render_* render with translucency on; off again on exit."""

    def __init__(self, lib, opaque_alpha=DEFAULT[0], max_crossings=DEFAULT[1], on=True):
        self.lib, self.args = lib, (1 if on else 0, float(opaque_alpha), int(max_crossings))

    def __enter__(self):
        self.lib.lib.glass_set(*self.args)
        return self

    def __exit__(self, *exc):
        self.lib.lib.glass_set(0, DEFAULT[0], DEFAULT[1])
        return False


_lib = None


def lib() -> GlassLib:
    global _lib
    if _lib is None:
        _build()
        _lib = GlassLib(LIB)
    return _lib


def render(sc, seeds, glass=DEFAULT, ext=None, max_depth=5, census=False, gids=None):
    """The specification's image of `sc` after `seeds` with translucency glass = (opaque_alpha, max_crossings) — None: off — and the
    extended options `ext` (PortExt's keywords), and — census=True — what its samples met."""
    L = lib()
    if census:
        L.census(enable=True, reset=True)
    try:
        g = Glass(L, on=False) if glass is None else Glass(L, *glass)
        with binding.PortExt(L, sc, **(ext or {})), binding.PortOptions(L, 256, max_depth, 13.0), g:
            img = L.glass_render_passes(sc, seeds) if gids is None else L.glass_render_gids(sc, seeds, gids)
        return (img, L.census(reset=True)) if census else img
    finally:
        if census:
            L.census(enable=False)
