"""Layout of gs_replay_frame and of the five argument structs that begin with
it, for the layout tests of the feature, contribution and distortion passes:
the C compiler's sizes and offsets, the ctypes mirror's, and the literals
below must agree.

The literals are the layout of the structs when each spelled the frame's
eleven fields out itself: sizeof / offsetof printed by a C program compiled
against the header of the commit before gs_replay_frame was introduced.  The
nested struct must occupy the same bytes (GS_ABI_VERSION did not move)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAME_SIZE = 176
FRAME = {"cam": 0, "tiles_x": 108, "tiles_y": 112, "ranges": 120, "sorted_gauss": 128, "records": 136,
         "cell_neval": 144, "live_bits": 152, "live_words": 160, "num_pairs": 168, "num_gaussians": 172}
# struct -> (its ctypes mirror, sizeof, the offsets of its own fields after the frame)
STRUCTS = {
    "gs_feature_fwd_args": ("GsFeatureFwdArgs", 200, {"channels": 176, "features": 184, "out": 192}),
    "gs_feature_bwd_args": ("GsFeatureBwdArgs", 232, {
        "channels": 176, "chunk": 180, "features": 184, "out": 192, "g_out": 200, "pair_grads": 208,
        "slot_live": 216, "cell_begin": 224, "cell_count": 228}),
    "gs_contrib_args": ("GsContribArgs", 216, {
        "partials": 176, "slot_live": 184, "cell_begin": 192, "cell_count": 196, "dominant_id": 200,
        "dominant_weight": 208}),
    "gs_distortion_fwd_args": ("GsDistortionFwdArgs", 216, {
        "near": 176, "far": 180, "distortion": 184, "moments": 192, "median_depth": 200, "median_id": 208}),
    "gs_distortion_bwd_args": ("GsDistortionBwdArgs", 232, {
        "near": 176, "far": 180, "distortion": 184, "moments": 192, "g_distortion": 200, "pair_grads": 208,
        "slot_live": 216, "cell_begin": 224, "cell_count": 228}),
}


def check(pkg, tmp_path, cnames):
    """Header, mirror and literals agree on gs_replay_frame and on `cnames`."""
    N = pkg._native
    assert C.sizeof(N.GsCamera) == 108 and C.sizeof(N.GsReplayFrame) == FRAME_SIZE
    assert [name for name, _ in N.GsReplayFrame._fields_] == list(FRAME)
    want = [FRAME_SIZE] + list(FRAME.values())
    mirror = [C.sizeof(N.GsReplayFrame)] + [getattr(N.GsReplayFrame, k).offset for k in FRAME]
    lines = ['P(sizeof(gs_replay_frame));'] + ['P(offsetof(gs_replay_frame, %s));' % k for k in FRAME]
    for cname in cnames:
        mname, size, own = STRUCTS[cname]
        t = getattr(N, mname)
        assert [name for name, _ in t._fields_] == ["f"] + list(own), cname
        want += [size, 0] + list(FRAME.values()) + list(own.values())
        # (the frame is anonymous in the mirror: t.cam is the field of t.f, at its offset in t)
        mirror += [C.sizeof(t), t.f.offset] + [getattr(t, k).offset for k in list(FRAME) + list(own)]
        lines += ['P(sizeof(%s));' % cname, 'P(offsetof(%s, f));' % cname]
        lines += ['P(offsetof(%s, f.%s));' % (cname, k) for k in FRAME]
        lines += ['P(offsetof(%s, %s));' % (cname, k) for k in own]
    src = tmp_path / "replay_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gsplat_mi355x.h"\n'
                   '#define P(x) printf("%zu\\n", (size_t)(x))\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "replay_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, "the header's layout is not the flat structs'"
    assert mirror == want, "the ctypes mirror's layout is not the flat structs'"
