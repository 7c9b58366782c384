"""Host-side validation of the layer-chain entry points (ptt_sa_fused_fwd_f32, ptt_rows_mlp_f32, ptt_xcorr_fused_fwd_f32): status
codes and the order in which the checks fire, with a null stream and host addresses that are never dereferenced. Every case
is refused before the first runtime call, so this needs no device."""
import ctypes

import pytest

from ptt_amd import _lib
from ptt_amd._lib import SaDesc, SaLayer, XcorrDesc

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4        # ptt_status (include/ptt_hip.h)

_buf = (ctypes.c_char * 256)()
PTR = (ctypes.addressof(_buf) + 15) & ~15           # a non-null, 16-byte aligned address; nothing reads it


@pytest.fixture(scope="module")
def lib():
    loaded = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ptt_sa_fused_fwd_f32", "ptt_rows_mlp_f32", "ptt_xcorr_fused_fwd_f32", "ptt_sa_compact_workspace"):
        fn = getattr(loaded, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    loaded.ptt_last_error_string.restype = ctypes.c_char_p
    return loaded


def _layers(dst, chain, wp=PTR):
    """dst[i] <- (Cin, Cout) of chain[i], ReLU, no separate scale."""
    for L, (cin, cout) in zip(dst, chain):
        L.Wpacked, L.scale, L.shift, L.Cin, L.Cout, L.relu = wp, None, None, cin, cout, 1


def _sa(chain, nsample=32, C=0, l0=0, B=2, M=64):
    d = SaDesc()
    d.xyz = d.new_xyz = d.idx = d.out = PTR
    d.feat = PTR if C else None
    d.feat_sb, d.feat_sc, d.feat_sn = C * 128, 128, 1
    d.out_sb, d.out_sc, d.out_sm = M * chain[-1][1], 1, chain[-1][1]
    d.B, d.N, d.M, d.nsample, d.C = B, 128, M, nsample, C
    d.radius, d.use_xyz, d.normalize_xyz, d.n_layers = 0.5, 1, 1, len(chain)
    _layers(d.layers, chain)
    if l0:
        d.l0_point_term = d.l0_xyz_weight = PTR
        d.l0_channels, d.l0_relu = l0, 1
    return d


SA0 = [(3, 64), (64, 64), (64, 128)]                # the persistent LDS-resident kernel's shape
STREAM = [(128, 128), (128, 256)]                   # the stream kernel's shape, behind a hoisted 128-channel layer 0
DENSE = [(19, 64), (64, 128), (128, 256)]           # 16 feature channels + xyz: sa_fused_kernel


def _sa_call(lib, d):
    rc = lib.ptt_sa_fused_fwd_f32(ctypes.byref(d), None)
    return rc, lib.ptt_last_error_string()


def test_sa_fused_layer_table(lib):
    d = _sa(DENSE, C=16)
    d.n_layers = 5
    rc, msg = _sa_call(lib, d)
    assert rc == EINVAL and b"ptt_sa_fused_fwd_f32" in msg and b"layers=5" in msg

    rc, msg = _sa_call(lib, _sa([(19, 64), (96, 128), (128, 256)], C=16))
    assert rc == EINVAL and b"ptt_sa_fused_fwd_f32: layer 1 Cin=96, expected 64" in msg

    for bad in (48, 288):
        rc, msg = _sa_call(lib, _sa([(19, 64), (64, bad), (bad, 256)], C=16))
        assert rc == EUNSUPPORTED and (b"ptt_sa_fused_fwd_f32: layer 1 Cout=%d must be a multiple of 32 <= 256" % bad) in msg

    d = _sa(DENSE, C=16)
    d.layers[2].Wpacked = None
    rc, msg = _sa_call(lib, d)
    assert rc == EINVAL and b"ptt_sa_fused_fwd_f32: layer 2 has no weights" in msg

    # layer 0 is checked before layer 1: its width wins over the broken chain behind it
    rc, msg = _sa_call(lib, _sa([(19, 48), (64, 128), (128, 256)], C=16))
    assert rc == EUNSUPPORTED and b"layer 0 Cout=48" in msg

    rc, msg = _sa_call(lib, _sa(DENSE, nsample=8, C=16))
    assert rc == EUNSUPPORTED and b"ptt_sa_fused_fwd_f32: nsample=8" in msg


@pytest.mark.parametrize("shape", ["sa0", "stream"])
def test_sa_fused_compact_workspace_is_the_last_check_before_the_launch(lib, shape):
    make = (lambda: _sa(SA0)) if shape == "sa0" else (lambda: _sa(STREAM, l0=128))
    need = lib.ptt_sa_compact_workspace(2, 64)
    assert need > 0
    d = make()
    d.compact_ws, d.compact_ws_bytes = PTR, need - 1             # one byte short
    rc, msg = _sa_call(lib, d)
    assert rc == EWORKSPACE and b"ptt_sa_fused_fwd_f32: compact_ws needs %d bytes" % need in msg
    d = make()
    d.compact_ws, d.compact_ws_bytes = PTR + 4, need             # misaligned by 4
    rc, msg = _sa_call(lib, d)
    assert rc == EWORKSPACE and b"16-byte aligned" in msg


def _rows(lib, chain, K=None, ldo=None, wp=PTR):
    arr = (SaLayer * len(chain))()
    _layers(arr, chain, wp)
    K = chain[0][0] if K is None else K
    ldo = chain[-1][1] if ldo is None else ldo
    rc = lib.ptt_rows_mlp_f32(PTR, 64, K, K, arr, len(chain), None, 0, PTR, ldo, None)
    return rc, lib.ptt_last_error_string()


def test_rows_mlp_layer_table(lib):
    rc, msg = _rows(lib, [(268, 256), (256, 256)])
    assert rc == EUNSUPPORTED and b"ptt_rows_mlp_f32: K=268" in msg
    rc, msg = _rows(lib, [(256, 288), (288, 256)])
    assert rc == EUNSUPPORTED and b"ptt_rows_mlp_f32: layer 0 Cout=288 (inner layers <= 256, the last <= 384)" in msg
    rc, msg = _rows(lib, [(256, 256), (256, 416)])
    assert rc == EUNSUPPORTED and b"ptt_rows_mlp_f32: layer 1 Cout=416" in msg
    rc, msg = _rows(lib, [(256, 256), (256, 259)], ldo=258)
    assert rc == EINVAL and b"ptt_rows_mlp_f32: ldo=258" in msg
    rc, msg = _rows(lib, [(256, 256), (128, 259)])
    assert rc == EINVAL and b"ptt_rows_mlp_f32: layer 1 Cin=128, expected 256" in msg
    # 384 passes the width check of the last layer (no launch is reached: ldo is refused after the table is built)
    rc, msg = _rows(lib, [(256, 256), (256, 384)], ldo=383)
    assert rc == EINVAL and b"ptt_rows_mlp_f32: ldo=383" in msg and b"Cout=384" in msg
    # any width below the cap passes too (rows_mlp pads to whole column tiles): Cout = 48 inside, 5 at the end
    rc, msg = _rows(lib, [(256, 48), (48, 5)], ldo=4)
    assert rc == EINVAL and b"ptt_rows_mlp_f32: ldo=4" in msg
    rc, msg = _rows(lib, [(256, 256), (256, 5)], wp=None)
    assert rc == EINVAL and b"ptt_rows_mlp_f32: layer 0 has no weights" in msg


def _xcorr(chain, Nt=64, C0=64, B=2, Ns=128, split=False):
    d = XcorrDesc()
    d.cos_t = d.P = d.w_sim = d.out = PTR
    d.out_sb, d.out_sc, d.out_sn = Ns * chain[-1][1], 1, chain[-1][1]
    d.B, d.Ns, d.Nt, d.C0, d.n_layers = B, Ns, Nt, C0, len(chain)
    _layers(d.layers, chain)
    if split:
        d.split, d.out_sh = 1, B * Ns * chain[-1][1]
        d.search_feat = d.templ_feat = PTR
        d.s_sb, d.s_sn, d.t_sb, d.t_sn, d.C, d.eps = Ns * 256, 256, Nt * 256, 256, 256, 1e-8
        d.cos_t = None
    return d


def test_xcorr_fused_layer_table(lib):
    call = lambda d: (lib.ptt_xcorr_fused_fwd_f32(ctypes.byref(d), None), lib.ptt_last_error_string())
    good = [(64, 128), (128, 256)]
    rc, msg = call(_xcorr(good, Nt=65))
    assert rc == EUNSUPPORTED and b"ptt_xcorr_fused_fwd_f32: Nt=65" in msg
    rc, msg = call(_xcorr([(64, 128)]))
    assert rc == EUNSUPPORTED and b"ptt_xcorr_fused_fwd_f32: needs at least two MFMA layers" in msg
    rc, msg = call(_xcorr([(12, 128), (128, 256)], C0=12))
    assert rc == EUNSUPPORTED and b"ptt_xcorr_fused_fwd_f32: C0=12" in msg
    rc, msg = call(_xcorr([(64, 128), (96, 256)]))
    assert rc == EINVAL and b"ptt_xcorr_fused_fwd_f32: layer 1 Cin=96, expected 128" in msg
    rc, msg = call(_xcorr([(64, 48), (48, 256)]))
    assert rc == EUNSUPPORTED and b"ptt_xcorr_fused_fwd_f32: layer 0 Cout=48" in msg
    d = _xcorr(good)
    d.layers[1].Wpacked = None
    rc, msg = call(d)
    assert rc == EINVAL and b"ptt_xcorr_fused_fwd_f32: layer 1 has no weights" in msg
    rc, msg = call(_xcorr(good, B=1, Ns=12, split=True))
    assert rc == EINVAL and b"ptt_xcorr_fused_fwd_f32: the split form" in msg
