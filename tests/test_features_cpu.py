"""The feature pass's C ABI without a GPU: its entry points reject bad
arguments before any HIP call, its structs' ctypes mirrors have the C
compiler's sizes, and the ABI version did not move (exports were only added)."""
import ctypes as C
import os
import subprocess

import replay_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _camera(a, width=40, height=24, tile=16):
    a.cam.image_width, a.cam.image_height, a.cam.tile_size = width, height, tile
    a.tiles_x, a.tiles_y = (width + tile - 1) // tile, (height + tile - 1) // tile


def test_abi_version_unchanged(pkg):
    assert pkg._native.load().gs_abi_version() == 23
    assert pkg._native.GS_FEATURE_CHUNK == 4 and pkg._native.GS_MAX_FEATURE_CHANNELS == 256


def test_feature_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    names = ["gs_feature_fwd_args", "gs_feature_bwd_args", "gs_feature_gather_args"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gsplat_mi355x.h"\nint main(){' +
                   "".join('printf("%%zu\\n", sizeof(%s));' % n for n in names) +
                   'printf("%d\\n%d\\n", GS_FEATURE_CHUNK, GS_MAX_FEATURE_CHANNELS);}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(N.GsFeatureFwdArgs), C.sizeof(N.GsFeatureBwdArgs), C.sizeof(N.GsFeatureGatherArgs),
                   N.GS_FEATURE_CHUNK, N.GS_MAX_FEATURE_CHANNELS]
    # every offset of the two structs that begin with the frame, and the bytes the flat structs had
    replay_layout.check(pkg, tmp_path, ["gs_feature_fwd_args", "gs_feature_bwd_args"])


def test_forward_rejects_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    assert lib.gs_blend_features_forward(None, None) == 1
    assert b"gs_blend_features_forward" in lib.gs_last_error() and b"null" in lib.gs_last_error()
    a = N.GsFeatureFwdArgs()
    for bad in (0, -1, N.GS_MAX_TILE + 1):
        _camera(a)
        a.cam.tile_size = bad
        assert lib.gs_blend_features_forward(C.byref(a), None) == 3
    _camera(a)
    a.tiles_x += 1  # a tile grid that is not the camera's
    a.channels = 4
    assert lib.gs_blend_features_forward(C.byref(a), None) == 1
    assert b"tiles_x" in lib.gs_last_error()
    _camera(a)
    for bad in (0, -3, N.GS_MAX_FEATURE_CHANNELS + 1):
        a.channels = bad
        assert lib.gs_blend_features_forward(C.byref(a), None) == 1
        assert b"channels" in lib.gs_last_error()
    a.channels = N.GS_MAX_FEATURE_CHANNELS  # in range: the NULL buffers are next
    assert lib.gs_blend_features_forward(C.byref(a), None) == 1
    assert b"null buffer" in lib.gs_last_error()


def test_backward_rejects_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    assert lib.gs_blend_features_backward(None, None) == 1
    assert b"gs_blend_features_backward" in lib.gs_last_error()
    a = N.GsFeatureBwdArgs()
    _camera(a)
    a.cam.tile_size = 0
    assert lib.gs_blend_features_backward(C.byref(a), None) == 3
    _camera(a, tile=24)  # 9 cells
    a.tiles_y += 2
    a.channels = 6
    assert lib.gs_blend_features_backward(C.byref(a), None) == 1
    _camera(a, tile=24)
    for bad in (0, N.GS_MAX_FEATURE_CHANNELS + 1):
        a.channels = bad
        assert lib.gs_blend_features_backward(C.byref(a), None) == 1
    a.channels = 6  # two chunks
    for bad in (-1, 2):
        a.chunk = bad
        assert lib.gs_blend_features_backward(C.byref(a), None) == 1
        assert b"chunk" in lib.gs_last_error()
    a.chunk = 1
    assert lib.gs_blend_features_backward(C.byref(a), None) == 1
    assert b"null buffer" in lib.gs_last_error()
    # the cell batch is checked once the buffers are there (never dereferenced: the call returns first)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p).value
    for name in ("ranges", "sorted_gauss", "records", "cell_neval", "features", "out", "g_out", "pair_grads",
                 "slot_live"):
        setattr(a, name, p)
    a.num_gaussians = 1
    for begin, count in ((-1, 2), (0, 10), (8, 2), (9, 1), (3, -1), (4, 0)):
        a.cell_begin, a.cell_count = begin, count
        assert lib.gs_blend_features_backward(C.byref(a), None) == 1, (begin, count)
        assert b"cell batch" in lib.gs_last_error()


def test_gather_rejects_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    assert lib.gs_gather_feature_partials(None, None) == 1
    assert b"gs_gather_feature_partials" in lib.gs_last_error()
    a = N.GsFeatureGatherArgs(n=4, partial_groups=4, channel_count=4, d_features_stride=8)
    assert lib.gs_gather_feature_partials(C.byref(a), None) == 1
    assert b"null buffer" in lib.gs_last_error()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p).value
    for name in ("vis", "rects", "pair_offset", "pair_grads", "slot_live", "grad_sums", "d_features"):
        setattr(a, name, p)
    a.partial_groups = 0
    assert lib.gs_gather_feature_partials(C.byref(a), None) == 1
    a.partial_groups = 4
    for begin, count, stride in ((0, 0, 8), (0, 5, 8), (-4, 4, 8), (8, 4, 8), (254, 4, 512), (0, 4, 3)):
        a.channel_begin, a.channel_count, a.d_features_stride = begin, count, stride
        assert lib.gs_gather_feature_partials(C.byref(a), None) == 1, (begin, count, stride)
    a.n = -1
    assert lib.gs_gather_feature_partials(C.byref(a), None) == 1
    a.n, a.channel_begin, a.channel_count, a.d_features_stride = 0, 0, 4, 4  # nothing to gather: no launch
    assert lib.gs_gather_feature_partials(C.byref(a), None) == 0


def test_stale_library_is_named(pkg, tmp_path, monkeypatch):
    """A library built before the feature exports has the same ABI number:
    load() says it is out of date instead of ctypes' AttributeError."""
    import pytest
    N = pkg._native
    src = tmp_path / "old.c"
    src.write_text("int gs_abi_version(void) { return %d; }\nconst char *gs_last_error(void) { return \"\"; }\n"
                   % N.GS_ABI_VERSION)
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.NativeLibraryError, match="out of date"):
        N.load(str(so))
