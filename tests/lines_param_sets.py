"""Parameter sets and seeded inputs for the ranked-lines tests under non-default gn_eval_params
(test infrastructure only): tests/test_lines_params.py measures on the CPU how many ties each set
forces, tests/test_gpu_lines_params.py ranks the same inputs on the GPU under the same sets.

The sets are built with eval_param_sets.make from that module's named overrides, plus one of this
module's own: "clamp0" (value_clamp = 0) makes every ordinary value 0, so that the order among
ordinary lines is the move order alone and a line drawn by rule ties with all of them.  The restated
rules (lines_rule, lines2_rule, history_rule, lines2_history_rule) read the oracle's current
parameters, so everything computed inside `under` follows the set.
"""
import contextlib

import eval_param_sets as S
import lines2_history_rule as H2
import lines2_rule as R2
import lines_rule as R

LINE_SETS = {
    "clamp0": dict(value_clamp=0),               # all ordinary values tie
    "rule50/clamp": S.NAMED["rule50/clamp"],     # many ties, not all
    "ties-poly": S.NAMED["ties-poly"],           # the defaults' order, every score another
    "material": S.NAMED["material"],             # another order, no mass ties
}
ALL_SMALL = "all small"                          # depth 1, mode FULL only: every position on the small net
N_RANDOM1, N_RANDOM2 = 128, 24
GAMES_SEED, N_GAMES, GAME_PLIES = 0x5EED11E6, 8, 40  # the seed of the other lines tests' random games


def overrides(name):
    return LINE_SETS[name] if name in LINE_SETS else S.NAMED[name]


@contextlib.contextmanager
def under(oracle_lib, name, ctx=None):
    """The oracle and, when given, the GPU context under the set `name` (None: the defaults); both
    back at their defaults afterwards.  Never held across a fixture's yield: whatever is computed
    under a set is computed and compared inside one `with`."""
    p = None if name is None else S.make(oracle_lib, overrides(name))  # (make resets the oracle itself)
    try:
        if p is not None:
            if ctx is not None:
                ctx.set_eval_params(S.as_gpu(p))
            oracle_lib.set_eval_params(p)
        yield p
    finally:
        oracle_lib.set_eval_params(None)
        if ctx is not None:
            from fishnet_amd import gpu_nnue as G
            ctx.set_eval_params(G.default_eval_params())


def depth1_fens():
    """tests/golden/lines_fens.txt, then the first 128 positions of test_gpu_lines.py's seeded set."""
    from fishnet_amd import gpu_nnue as G
    return R.fixture_fens() + G.boards_to_fens(G.random_positions(R.SEED, 0, N_RANDOM1, 160))


def depth2_fens():
    """tests/golden/lines2_fens.txt, then the first 24 positions of test_gpu_lines2.py's seeded set."""
    from fishnet_amd import gpu_nnue as G
    return R2.fixture_fens() + G.boards_to_fens(G.random_positions(R2.SEED, 0, N_RANDOM2, 160))


def history_games():
    """The 15 games of both history fixtures: [(root_fen, uci_moves, skip)]."""
    return H2.both_fixtures()


def random_games():
    """8 seeded games of 40 plies from the start position, nothing skipped."""
    from fishnet_amd import gpu_nnue as G
    return [(R.START, u, ()) for u in G.random_games_uci(GAMES_SEED, 0, N_GAMES, GAME_PLIES)]
