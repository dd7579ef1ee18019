"""The fused engine's choice of gradient exchange (engine/xchg_selftest.choose_exchange) as
a decision table on the CPU.  The two callbacks are collectives in the engine, so besides
the outcome each row pins the exact sequence of calls: a rank that made another sequence
would hang the gang.  Expected values are written out by hand from the rules."""
import pytest

from distributed_amd.engine.xchg_selftest import choose_exchange

S, P, R = "xgmi-sharded", "xgmi-peer", "rccl"
US = 1e-6


def _row(id, mode="auto", world=2, exclude=(), rccl=False, selftested=True, tune=True, passes=(), times=None,
         verify=(), time=(), chosen=None, verified=None, fallback=(), us=None):
    return pytest.param(dict(mode=mode, world=world, exclude=set(exclude), rccl=rccl, selftested=selftested, tune=tune,
                             passes=set(passes), times=times or {}, verify=list(verify), time=list(time),
                             chosen=chosen, verified=verified, fallback=list(fallback), us=us or {}), id=id)


ROWS = [
    _row("a-tuned-all-pass-sharded-fastest", rccl=True, passes=(S, P), times={S: 30 * US, P: 40 * US, R: 50 * US},
         verify=[S, P], time=[S, P, R], chosen=S, verified=True, us={S: 30.0, P: 40.0, R: 50.0}),
    _row("b-tuned-rccl-fastest", rccl=True, passes=(S, P), times={S: 30 * US, P: 40 * US, R: 20 * US},
         verify=[S, P], time=[S, P, R], chosen=R, verified=None, us={S: 30.0, P: 40.0, R: 20.0}),
    _row("c-tuned-sharded-fails-no-rccl", passes=(P,), verify=[S, P], time=[], chosen=P, verified=True, fallback=[S]),
    _row("d-tuned-sharded-fails-rccl", rccl=True, passes=(P,), times={P: 40 * US, R: 50 * US},
         verify=[S, P], time=[P, R], chosen=P, verified=True, fallback=[S], us={P: 40.0, R: 50.0}),
    _row("e-tuned-both-fail-rccl", rccl=True, verify=[S, P], time=[], chosen=None, fallback=[S, P]),
    _row("e-tuned-both-fail-no-rccl", verify=[S, P], time=[], chosen=None, fallback=[S, P]),
    _row("f-untuned-sharded-passes", rccl=True, tune=False, passes=(S, P), verify=[S], chosen=S, verified=True),
    _row("g-untuned-sharded-fails", rccl=True, tune=False, passes=(P,), verify=[S, P], chosen=P, verified=True,
         fallback=[S]),
    _row("h-sharded-pinned-pass", mode="sharded", rccl=True, passes=(S, P), verify=[S], chosen=S, verified=True),
    _row("h-sharded-pinned-fail", mode="sharded", rccl=True, passes=(P,), verify=[S], chosen=None, fallback=[S]),
    _row("i-xgmi-pinned-pass", mode="xgmi", rccl=True, passes=(S, P), verify=[P], chosen=P, verified=True),
    _row("i-xgmi-pinned-fail", mode="xgmi", rccl=True, passes=(S,), verify=[P], chosen=None, fallback=[P]),
    _row("j-world-9", world=9, passes=(S, P), verify=[P], chosen=P, verified=True),
    _row("k-sharded-excluded", exclude={S}, rccl=True, passes=(S, P), times={P: 40 * US, R: 50 * US},
         verify=[P], time=[P, R], chosen=P, verified=True, us={P: 40.0, R: 50.0}),
    _row("k-both-excluded", exclude={S, P}, rccl=True, passes=(S, P), times={R: 50 * US}, chosen=None),
    _row("l-no-selftest-tuned", rccl=True, selftested=False, times={S: 30 * US, P: 25 * US, R: 50 * US},
         time=[S, P, R], chosen=P, verified=None, us={S: 30.0, P: 25.0, R: 50.0}),
    _row("l-no-selftest-untuned", rccl=True, selftested=False, tune=False, chosen=S, verified=None),
    _row("m-tuned-nothing-timed", rccl=True, passes=(S, P), verify=[S, P], time=[S, P, R], chosen=S, verified=True),
    _row("n-tuned-sharded-not-timed", rccl=True, passes=(S, P), times={P: 40 * US, R: 35 * US},
         verify=[S, P], time=[S, P, R], chosen=R, verified=None, us={P: 40.0, R: 35.0}),
]


@pytest.mark.parametrize("row", ROWS)
def test_choose_exchange(row):
    calls = {"verify": [], "time": []}

    def verify(kind):
        calls["verify"].append(kind)
        return kind in row["passes"]

    def time(kind):
        calls["time"].append(kind)
        return row["times"].get(kind)

    chosen, verified, fallback, us = choose_exchange(row["mode"], row["world"], row["exclude"], row["rccl"],
                                                     row["selftested"], row["tune"], verify, time)
    assert calls == {"verify": row["verify"], "time": row["time"]}
    assert chosen == row["chosen"]
    assert verified is row["verified"]
    assert fallback == row["fallback"]
    assert us == row["us"]
