"""saicv_c3_bwd_stream_ok (csrc/c3bwd.hip): which layers take the fused c3 backward is a pure function of (dtype, M, CO, CI) and of
the two switches SAICV_C3_BWD_STREAM / SAICV_C3_BWD_MIN_ROWS, read per call.  Host only: nothing reaches a GPU."""
import pytest

BF16, F32 = 0, 1
STAGE1 = (256 * 56 * 56, 256, 64)
STAGE2 = (256 * 28 * 28, 512, 128)


@pytest.fixture
def ok(monkeypatch):
    from simpleaicv_pytorch_training_examples_amd import _lib
    monkeypatch.delenv('SAICV_C3_BWD_STREAM', raising=False)
    monkeypatch.delenv('SAICV_C3_BWD_MIN_ROWS', raising=False)
    return _lib.lib().saicv_c3_bwd_stream_ok, _lib.lib().saicv_c3_bwd_stream_rows, monkeypatch


def test_defaults(ok):
    ok, rows, _ = ok
    assert ok(BF16, *STAGE1) == rows(*STAGE1) == 512            # rows of partial sums: those of the streaming data gradient
    assert ok(BF16, 65536, 256, 64) == 512 and ok(BF16, 65535, 256, 64) == 0      # stages 3-4 and small batches stay as they are
    assert ok(F32, *STAGE1) == 0
    for co, ci in ((256, 128), (64, 64), (1024, 256), (2048, 512), (64, 256), (128, 512)):
        assert ok(BF16, 802816, co, ci) == 0 and rows(802816, co, ci) == 0
    assert ok(BF16, 0, 256, 64) == 0 and ok(BF16, -5, 256, 64) == 0
    # buffer-addressed operands stay below 4 GiB, the last tile's rows included
    assert rows((1 << 32) // 512 - 64, 256, 64) > 0 and rows((1 << 32) // 512 - 32, 256, 64) == 0
    # the (512, 128) form exists (the launch takes it) whatever the routing decides for it
    assert rows(*STAGE2) == 512 and ok(BF16, *STAGE2) == 0


def test_pure_and_repeatable(ok):
    ok, _, _ = ok
    args = (BF16, *STAGE1)
    assert len({ok(*args) for _ in range(5)}) == 1


def test_switches_are_read_per_call(ok):
    ok, rows, mp = ok
    mp.setenv('SAICV_C3_BWD_STREAM', '0')
    assert ok(BF16, *STAGE1) == 0 and rows(*STAGE1) == 512      # the launch itself ignores the switches
    mp.setenv('SAICV_C3_BWD_STREAM', '1')
    assert ok(BF16, *STAGE1) == 512
    mp.setenv('SAICV_C3_BWD_MIN_ROWS', '0')
    assert ok(BF16, 98, 256, 64) == 2 and ok(BF16, 32, 256, 64) == 1 and ok(BF16, 2304, 256, 64) == 36
    mp.setenv('SAICV_C3_BWD_MIN_ROWS', '1000000')
    assert ok(BF16, *STAGE1) == 0
    mp.delenv('SAICV_C3_BWD_MIN_ROWS')
    assert ok(BF16, *STAGE1) == 512
