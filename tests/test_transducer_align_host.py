"""CPU-side checks of transducer forced alignment (no GPU): the exported symbols, every argument check of the two entries (they
run before any launch), the workspace size and the hybrid model's keyword."""
import ctypes

import pytest


def test_symbols_are_exported_and_declared():
    from nemo_amd import _lib, modules, ops
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mi355x_transducer_align_rows", "mi355x_transducer_align", "mi355x_transducer_align_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and name in _lib.SIGNATURES, name
    assert hasattr(modules, "TransducerAligner") and hasattr(ops, "transducer_align") and hasattr(ops, "transducer_align_rows")


def test_workspace_size():
    from nemo_amd import _lib
    size = _lib.lib.mi355x_transducer_align_workspace_bytes
    for U1, cells in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (257, 8), (513, 16), (1024, 16)):
        assert size(3, 7, U1) == 3 * (7 + U1 - 1) * 64 * cells, U1   # one byte per cell, diagonals padded to the wave's columns
    assert [size(0, 7, 5), size(3, 0, 5), size(3, 7, 0), size(3, 7, 1025)] == [-1] * 4


def test_invalid_arguments_are_rejected_without_a_gpu():
    """rc 1 = MI_ERR_ARG.  Non-null dummy pointers are never dereferenced on the host."""
    from nemo_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    dur = lambda *d: (ctypes.c_int * len(d))(*d)

    def rows(ptrs=(p,) * 5, **kw):   # pointers: acts, labels, act_lens, label_lens, rows
        z = dict(dict(ld=12, B=1, T=4, U1=3, V1=5, D=0, blank=4), **kw)
        return L.mi355x_transducer_align_rows(ptrs[0], z["ld"], *ptrs[1:4], z["B"], z["T"], z["U1"], z["V1"], z["D"], z["blank"],
                                              ptrs[4], None)

    def lattice(ptrs=(p,) * 6, durations=None, ws_bytes=1 << 20, **kw):   # rows, act_lens, label_lens, ws, tok_frame, tok_dur (, score)
        z = dict(dict(D=0, B=1, T=4, U1=3), **kw)
        return L.mi355x_transducer_align(*ptrs[:3], durations, z["D"], z["B"], z["T"], z["U1"], ptrs[3], ws_bytes, *ptrs[4:6],
                                         kw.get("score", p), None)
    for i in range(5):
        assert rows([None if j == i else p for j in range(5)]) == 1, i
    for kw in (dict(B=0), dict(T=0), dict(U1=0), dict(U1=1025), dict(V1=1), dict(blank=-1), dict(blank=5), dict(D=1), dict(D=9),
               dict(D=-1), dict(ld=4), dict(D=5, ld=9)):
        assert rows(**kw) == 1, kw
    for i in range(6):
        assert lattice([None if j == i else p for j in range(6)]) == 1, i
    assert lattice(score=None) == 1
    for kw in (dict(B=0), dict(T=0), dict(U1=0), dict(U1=1025), dict(D=3), dict(ws_bytes=6 * 64 - 1), dict(durations=dur(0, 1)),
               dict(D=2, durations=dur(1, 2)), dict(D=2, durations=dur(0, 9)), dict(D=3, durations=dur(0, 2, 2)),
               dict(D=1, durations=dur(0)), dict(D=2, durations=dur(0, 5), U1=257),   # (a largest duration above 4: U1 <= 256)
               dict(ptrs=(p, p, p, p + 8, p, p))):   # (the last: a misaligned workspace)
        assert lattice(**kw) == 1, kw
    with pytest.raises(ValueError):
        _lib.check(lattice(B=0), "transducer_align")


def test_hybrid_align_keyword_is_validated():
    from nemo_amd.models import EncDecHybridRNNTCTCModel
    import inspect
    assert inspect.signature(EncDecHybridRNNTCTCModel.align).parameters["decoder_type"].default == "ctc"
    with pytest.raises(ValueError, match="decoder_type=beam"):
        EncDecHybridRNNTCTCModel.align(None, [], [], decoder_type="beam")
