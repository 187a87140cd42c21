"""The epoch-wrap tests' start values against the library's own limits, without a GPU: a start
value outside the range the experiment build accepts fails engine creation on the GPU, and one
that was silently replaced (UVHTTP_WS_EPOCH_START=(1 << 30) - 4, past kMaxHostEpoch) is how
test_epoch_wraparound came to run nowhere near the wrap."""
import uvhttp_amd as U

import test_gpu_epoch_wrap as W
import test_gpu_parity as P


def test_limits_split_the_tag_space():
    max_host, max_epoch = U.epoch_limits()
    # 30-bit tags ((epoch << 2) | kind fits a 32-bit word), the lower half the host's
    assert max_epoch == (1 << 30) - 1 and max_host == max_epoch // 2


def test_start_values_lie_inside_the_limits():
    max_host, max_epoch = U.epoch_limits()
    s = dict(W.starts())
    s["UVHTTP_WS_EPOCH_START"] = s["UVHTTP_WS_EPOCH_START"] + [P.wrap_start()]
    assert s["UVHTTP_WS_EPOCH_START"] and s["UVHTTP_WS_DEV_EPOCH_START"] and s["UVHTTP_WS_EPOCH_PERIOD"]
    for v in s["UVHTTP_WS_EPOCH_START"]:
        assert 0 <= v <= max_host - 1, v
        assert max_host - v <= 6  # (the tests run at least six calls: they cross the wrap)
    for v in s["UVHTTP_WS_DEV_EPOCH_START"]:
        assert max_host + 1 <= v <= max_epoch, v
        assert max_epoch - v < 8  # (eight replays)
    for v in s["UVHTTP_WS_EPOCH_PERIOD"]:
        assert 2 <= v <= max_host
        assert v % 3 and 3 * v < 16  # coprime with the 3-call pattern, three cycles in 16 calls


def test_experiment_knobs_name_the_epoch_hooks():
    for k in ("UVHTTP_WS_EPOCH_START", "UVHTTP_WS_EPOCH_PERIOD", "UVHTTP_WS_DEV_EPOCH_START"):
        assert k in U.EXPERIMENT_KNOBS
        assert k.encode() in open(U.TESTHOOKS_LIB_PATH, "rb").read()
    # (tests/test_abi.py checks that the product library names none of EXPERIMENT_KNOBS)
    prod = open(U.LIB_PATH, "rb").read()
    assert b"uvhttp_ws_gpu_test_epoch_limits" not in prod
    assert b"uvhttp_ws_gpu_test_engine_epochs" not in prod
