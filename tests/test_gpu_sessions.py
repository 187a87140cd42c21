"""Whole server sessions over many device calls, all state carried (tests/_session_ref.py): one
TlsEngine and one GpuEngine for a whole session, every call the chain open_records -> ws_streams ->
decode_reads -> validate_utf8_streams -> control_replies_streams -> echo_messages_streams ->
seal_frames (echoes) -> seal_frames (replies) on one stream with one host read at its end, and
between two calls the six things a server carries per connection: leftover ciphertext and read
sequence number, buffered WebSocket bytes, fragment state, the open UTF-8 sequence, the open
message's bytes (d_open -> d_carry) and the write sequence number.  The scripts, seeds and
schedules are those of test_session_host.py.  After every call every device output is compared
field for field and byte for byte with the host backend's for that call (TLS results and records,
stream table and results, delivered descriptors, decoded wire, verdicts and summary, reply and
echo conn / summary / out / out_off / runs, d_open / d_open_off, send results and sealed bytes);
at the end the one-shot assertions of the host file: cut invariance."""
import pytest

import _session_ref as SR
from test_gpu_epoch_wrap import _engine
from test_session_host import SEEDS, _expects, check_every_cut_conditions, check_random_conditions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def engines(torch):
    import uvhttp_amd as U
    tls, ws = U.TlsEngine(0), U.GpuEngine(0)
    yield tls, ws
    ws.close()
    tls.close()


def _both(torch, engines, conns, scheds, expects=None, backend=None):
    """the session on the host, then on the device against the host's log call by call, then the
    one-shot assertions on the device's connections"""
    _, host_log = SR.run_session(SR.HostBackend(), conns, scheds)
    backend = backend or SR.DeviceBackend(torch, *engines)
    lives, log = SR.run_session(backend, conns, scheds, expect_log=host_log)
    assert len(log) == len(host_log)
    return lives, log, SR.check_session(conns, scheds, lives, expects=expects)


@pytest.mark.parametrize("transport", ["plain", "tls"])
def test_every_cut_two_calls(torch, engines, transport):
    conns, scheds = SR.every_cut_session(transport)
    lives, log, expects = _both(torch, engines, conns, scheds)
    check_every_cut_conditions(conns, scheds, log)
    assert all(e.why == "closed" and e.leave_call == 1 for e in expects)


@pytest.mark.parametrize("transport", ["plain", "tls"])
@pytest.mark.parametrize("seed", SEEDS)
def test_random_sessions(torch, engines, seed, transport):
    if seed == 0:
        check_random_conditions(transport)
    conns, scheds, expects = _expects(seed, transport)
    _both(torch, engines, conns, scheds, expects)


def test_long_open_message_many_calls(torch, engines):
    conns, scheds = SR.long_open_session()
    lives, log, expects = _both(torch, engines, conns, scheds)
    SR.check_long_open_conditions(conns, scheds, log, expects)


class FreshEngines(SR.DeviceBackend):
    """a new pair of engines for every call"""

    def call(self, x):
        import uvhttp_amd as U
        self.tls, self.ws = U.TlsEngine(0), U.GpuEngine(0)
        try:
            return super().call(x)
        finally:
            self.ws.close()
            self.tls.close()


def test_shapes_shrink_and_grow(torch, engines):
    """300, 3, 600 and 1 live connections on the same engines: scratch grown, mostly unused,
    regrown.  Against the host, and output for output against fresh engines per call"""
    conns, scheds = SR.shapes_session()
    lives, log, _ = _both(torch, engines, conns, scheds)
    assert [x["S"] for x, _ in log] == [300, 3, 600, 1]
    SR.run_session(FreshEngines(torch, None, None), conns, scheds, expect_log=log)


@pytest.mark.parametrize("n", [1, 3])
def test_session_in_grid_pieces(torch, monkeypatch, n):
    """a random session with every chunked pass of the WebSocket engine going out in launches of n
    workgroups (UVHTTP_WS_GRID_PIECE, the experiment build)"""
    import uvhttp_amd as U
    ws = _engine(monkeypatch, {"UVHTTP_WS_GRID_PIECE": n})
    tls = U.TlsEngine(0)
    try:
        conns, scheds, expects = _expects(0, "tls")
        ws.grid_pieces()
        _both(torch, (tls, ws), conns, scheds, expects)
        passes, pieces, tiles = ws.grid_pieces()
        assert pieces > passes and tiles >= 5
    finally:
        ws.close()
        tls.close()
