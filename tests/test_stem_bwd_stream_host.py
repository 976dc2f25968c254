"""saicv_stem_bwd_stream_ok (csrc/stembwd.hip): which parts of the streamed backward a pooled stem block takes is a pure function of
(dtype, N, H, W, CO, CQ, R, S, pool) -- H, W the convolution output -- and of the two switches SAICV_STEM_BWD_STREAM /
SAICV_STEM_BWD_MIN_ROWS, read per call.  Bit 0 (KEEP): the forward keeps the maxima and the sums come from them; bit 1: the stream
kernel as well.  The stream kernel measured slower than the two kernels it replaces and is left unrouted: the default takes bit 0
alone, SAICV_STEM_BWD_STREAM=2 both.  Host only: nothing reaches a GPU."""
import pytest

BF16, F32 = 0, 1
KEEP, BOTH = 1, 3
STEM = (256, 112, 112, 64, 16, 4, 4, 3, 2, 1)          # ResNet-50 at batch 256: 3 211 264 rows


@pytest.fixture
def ok(monkeypatch):
    from simpleaicv_pytorch_training_examples_amd import _lib
    monkeypatch.delenv('SAICV_STEM_BWD_STREAM', raising=False)
    monkeypatch.delenv('SAICV_STEM_BWD_MIN_ROWS', raising=False)
    return _lib.lib().saicv_stem_bwd_stream_ok, monkeypatch


def _with(**kw):
    names = ('N', 'H', 'W', 'CO', 'CQ', 'R', 'S', 'pk', 'ps', 'pp')
    d = dict(zip(names, STEM))
    d.update(kw)
    return tuple(d[n] for n in names)


def test_defaults(ok):
    ok, _ = ok
    assert ok(BF16, *STEM) == KEEP
    # the minimum is 65 536 rows: small batches and small images keep today's launches
    assert ok(BF16, *_with(N=8, H=64, W=128)) == KEEP and ok(BF16, *_with(N=8, H=64, W=127)) == 0
    assert ok(BF16, *_with(N=6)) == KEEP and ok(BF16, *_with(N=5)) == 0


def test_every_refusal(ok):
    ok, _ = ok
    assert ok(F32, *STEM) == 0 and ok(2, *STEM) == 0
    for kw in (dict(CO=32), dict(CO=128), dict(CQ=8), dict(CQ=32), dict(R=3), dict(S=3), dict(R=7, S=7), dict(R=1, S=1),
               dict(pk=2), dict(pk=5), dict(ps=1), dict(ps=3), dict(pp=0), dict(pp=2)):
        assert ok(BF16, *_with(**kw)) == 0, kw
    for kw in (dict(N=0), dict(N=-1), dict(H=0), dict(H=-112), dict(W=0), dict(W=-3)):
        assert ok(BF16, *_with(**kw)) == 0, kw
    # buffer-addressed operands stay below 4 GiB, the 32 rows of the last step included: (M + 32) * 128 bytes of y
    edge = (0xfffffff0 - 1) // 128 - 32
    assert ok(BF16, *_with(N=1, H=1, W=edge)) == KEEP and ok(BF16, *_with(N=1, H=1, W=edge + 1)) == 0
    # ... and the space-to-depth image: N * (H + 3) * (W + 3) * 32 bytes (1 x 1 outputs: 512 bytes of image against 128 of y)
    assert ok(BF16, *_with(N=1 << 23, H=1, W=1)) == 0 and ok(BF16, *_with(N=1 << 22, H=1, W=1)) == KEEP


def test_pure_and_repeatable(ok):
    ok, _ = ok
    assert len({ok(BF16, *STEM) for _ in range(5)}) == 1


def test_switches_are_read_per_call(ok):
    ok, mp = ok
    mp.setenv('SAICV_STEM_BWD_STREAM', '0')
    assert ok(BF16, *STEM) == 0
    mp.setenv('SAICV_STEM_BWD_STREAM', '1')
    assert ok(BF16, *STEM) == KEEP
    mp.setenv('SAICV_STEM_BWD_STREAM', '2')
    assert ok(BF16, *STEM) == BOTH and ok(F32, *STEM) == 0 and ok(BF16, *_with(CO=128)) == 0 and ok(BF16, *_with(N=5)) == 0
    mp.setenv('SAICV_STEM_BWD_MIN_ROWS', '0')
    assert ok(BF16, *_with(N=2, H=17, W=24)) == BOTH and ok(BF16, *_with(N=1, H=1, W=1)) == BOTH
    mp.delenv('SAICV_STEM_BWD_STREAM')
    assert ok(BF16, *_with(N=2, H=17, W=24)) == KEEP
    assert ok(F32, *_with(N=2, H=17, W=24)) == 0
    mp.setenv('SAICV_STEM_BWD_MIN_ROWS', '10000000')
    assert ok(BF16, *STEM) == 0
    mp.delenv('SAICV_STEM_BWD_MIN_ROWS')
    assert ok(BF16, *STEM) == KEEP
