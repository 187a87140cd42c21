"""for_grid_chunks (ws_engine_int.h) on the host, without a GPU: a pass of `tiles` workgroups goes
out in launches of at most `piece`, each handed its first workgroup's index in the whole pass.
The split is run through the experiment build's uvhttp_ws_gpu_test_grid_chunks (the library's own
loop, not a restatement) at the product's piece of 2^24 and at the small pieces the GPU tests set
through UVHTTP_WS_GRID_PIECE; the 2^32 + 5 case is the one place an index past 32 bits is
exercised, since no test can launch that many workgroups."""
import pytest

import uvhttp_amd as U

import test_gpu_grid_pieces as G

P24 = 1 << 24


def _cases():
    out = []
    for piece in (1, 3, P24):
        tiles = [0, 1, piece - 1, piece, piece + 1]
        if piece == P24:
            tiles += [5 * piece - 123, (1 << 32) + 5]
        out += [(piece, t) for t in sorted(set(tiles))]
    return out


def test_product_piece_is_2_24():
    assert U.max_grid() == P24


@pytest.mark.parametrize("piece,tiles", _cases())
def test_pieces_cover_the_pass_once(piece, tiles):
    want = -(-tiles // piece)
    assert want <= 300
    n, pairs = U.grid_chunks(piece, tiles, cap=512)
    assert n == want == len(pairs)           # ceil(tiles / piece) launches, none for an empty pass
    base = 0
    for grid, tb in pairs:
        assert 1 <= grid <= piece            # non-empty, within the piece
        assert tb == base                    # contiguous from 0, in order
        base += grid
    assert base == tiles                     # every workgroup once, none past the end
    if pairs:                                # all but the last are full
        assert all(g == piece for g, _ in pairs[:-1])


def test_more_launches_than_the_array_holds_are_counted_not_written():
    n, pairs = U.grid_chunks(1, 10, cap=4)
    assert n == 10 and pairs == [(1, 0), (1, 1), (1, 2), (1, 3)]


def test_piece_values_of_the_gpu_tests_are_accepted():
    vals = G.pieces()
    assert vals and 1 in vals                # (a piece of one workgroup: tile_base = every index)
    for v in vals:
        assert 1 <= v <= U.max_grid(), v
        assert v < 5                         # the tests' passes have >= 5 tiles: always >= 2 pieces


def test_experiment_knobs_name_the_piece_hook():
    assert G.KNOB == "UVHTTP_WS_GRID_PIECE" and G.KNOB in U.EXPERIMENT_KNOBS
    assert G.KNOB.encode() in open(U.TESTHOOKS_LIB_PATH, "rb").read()
    # (tests/test_abi.py checks that the product library names none of EXPERIMENT_KNOBS)
    prod = open(U.LIB_PATH, "rb").read()
    for hook in (b"uvhttp_ws_gpu_test_grid_pieces", b"uvhttp_ws_gpu_test_grid_chunks",
                 b"uvhttp_ws_gpu_test_max_grid"):
        assert hook not in prod
