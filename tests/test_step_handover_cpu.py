"""The pre-step's hand-over decision (``csrc/step.hip``: ``step_handover``, queried through ``pmc_step_handover``) on
hand-filled ``pmc_step_t`` descriptors: where x', the finite mask, logp', the row count and the completion word go.  The
function reads fields and follows no pointer, so the addresses are fakes and none of this needs a GPU.

The reference is a restatement of the rules as ``pmc_step_pre`` had them before the decision had one place -- three places
of ``csrc/step.hip`` at commit ea2886d, cited line by line below -- over the full grid of the twelve switches they read."""
import ctypes as C
import itertools

import pytest

SWITCHES = ("host_direct", "p_xT", "lik_x", "prior", "prior_rows", "h_done", "done_ticket", "h_clean", "clean_count",
            "fill_rejected", "h_x", "epilogue")
# distinct fake addresses, nothing is dereferenced
ADDR = dict(p_xT=0x1000, lik_x=0x2000, prior=0x3000, h_done=0x4000, done_ticket=0x5000, h_clean=0x6000, clean_count=0x7000,
            h_x=0x8000, h_fin=0x9000, h_logp_out=0xA000, cur_x=0xB000, p_x=0xC000, p_logp=0xD000, h_logp=0xE000)
HOST = {ADDR[k] for k in ("h_done", "h_clean", "h_x", "h_fin", "h_logp_out", "h_logp")}
STEP = 41
FIELDS = ("x_colmajor", "finite_copy", "logp_copy", "done_ticket", "done_flag", "done_value", "bad_count", "bad_flag", "fill_x")
COPIES, DIRECT, DEVLIK = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


def descriptor(sw):
    from pocomc_amd import _lib
    s = _lib.pmc_step_t(n=21, D=5, h_fin=ADDR["h_fin"], h_logp_out=ADDR["h_logp_out"], h_logp=ADDR["h_logp"],
                        p_x=ADDR["p_x"], p_logp=ADDR["p_logp"])
    s.cur.x = ADDR["cur_x"]
    for k in ("host_direct", "prior_rows", "fill_rejected"):
        setattr(s, k, int(sw[k]))
    for k in ("p_xT", "lik_x", "prior", "h_done", "done_ticket", "h_clean", "clean_count", "h_x"):
        setattr(s, k, ADDR[k] if sw[k] else None)
    return s


def query(lib, sw):
    from pocomc_amd import _lib
    s, h, mode, unknown = descriptor(sw), _lib.pmc_handover_t(), C.c_int32(-7), C.c_int32(-7)
    assert lib.pmc_step_handover(C.byref(s), STEP, int(sw["epilogue"]), C.byref(h), C.byref(mode), C.byref(unknown)) == 0
    return {k: getattr(h, k) or 0 for k in FIELDS}, mode.value, unknown.value


def parent_rules(sw):
    """``pmc_step_pre`` of commit ea2886d, by line of its ``csrc/step.hip``; 0 is NULL."""
    a = lambda k: ADDR[k] if sw[k] else 0
    direct = bool(sw["host_direct"] and not sw["p_xT"])                                        # :75
    devlik = bool(sw["lik_x"] and (sw["prior"] or sw["prior_rows"]))                           # :94
    xT = a("lik_x") if devlik else a("h_x") if direct else a("p_xT")                           # :96
    fin2 = ADDR["h_fin"] if (direct and not devlik) else 0                                     # :97
    lp2 = ADDR["h_logp_out"] if (direct and sw["prior"] and not devlik) else 0                 # :98
    done = bool(direct and not devlik and sw["h_done"] and sw["done_ticket"])                  # :99-100
    ticket, flag, value = (ADDR["done_ticket"], ADDR["h_done"], STEP + 1) if done else (0, 0, 0)      # :124-126, :807-808 of mcmc_kernels.hip
    if sw["epilogue"]:
        bad_count = a("clean_count") if (done and sw["h_clean"]) else 0                        # :127
        bad_flag = a("h_clean") if (done and sw["h_clean"] and sw["clean_count"]) else 0       # :128
        fill_x = ADDR["cur_x"] if (sw["fill_rejected"] and bad_flag and xT) else 0             # :132
    else:
        counted = bool(done and sw["h_clean"] and sw["clean_count"] and xT and sw["prior"])    # :152 with scaled = false
        bad_count, bad_flag, fill_x = ((a("clean_count"), a("h_clean"), ADDR["cur_x"] if sw["fill_rejected"] else 0)
                                       if counted else (0, 0, 0))                              # :153
    if devlik:
        bad_count, bad_flag, fill_x = a("clean_count"), 0, ADDR["cur_x"]                       # :133, :154
    counted = bool(done and sw["h_clean"] and sw["clean_count"] and xT and (sw["epilogue"] or sw["prior"]))    # :152
    unknown = int(bool(sw["h_clean"]) and not counted)                                         # :155
    mode = DEVLIK if devlik else DIRECT if direct else COPIES                                  # :172: no copies follow unless COPIES
    h = dict(x_colmajor=xT, finite_copy=fin2, logp_copy=lp2, done_ticket=ticket, done_flag=flag, done_value=value,
             bad_count=bad_count, bad_flag=bad_flag, fill_x=fill_x)
    return h, mode, unknown


def grid():
    for bits in itertools.product((0, 1), repeat=len(SWITCHES)):
        yield dict(zip(SWITCHES, bits))


def test_the_decision_is_the_parents_over_the_whole_grid(lib):
    n, modes, unknowns = 0, set(), set()
    for sw in grid():
        got, want = query(lib, sw), parent_rules(sw)
        assert got == want, sw
        n += 1
        modes.add(got[1])
        unknowns.add(got[2])
    assert n == 4096 and modes == {COPIES, DIRECT, DEVLIK} and unknowns == {0, 1}


def test_grid_invariants(lib):
    seen = set()
    for sw in grid():
        h, mode, unknown = query(lib, sw)
        if h["done_flag"]:
            assert h["done_ticket"] and h["done_value"] == STEP + 1, sw        # no completion word without a ticket
        else:
            assert not h["done_ticket"] and h["done_value"] == 0, sw
        if h["bad_flag"]:
            assert h["done_flag"] and h["bad_count"], sw                       # the count travels with the completion word
        if mode == DEVLIK:
            assert not {h[k] for k in FIELDS if k != "done_value"} & HOST, sw   # nothing points at host memory
            assert h["x_colmajor"] == ADDR["lik_x"] and h["fill_x"] == ADDR["cur_x"], sw
        if h["fill_x"]:
            assert h["x_colmajor"], sw                                         # a fill needs the copy it fills
        if mode == COPIES:
            assert not {h[k] for k in FIELDS if k != "done_value"} & HOST, sw   # the stream's copies take everything over
        if not sw["h_clean"]:
            assert unknown == 0 and not h["bad_flag"], sw
        else:
            assert unknown == 1 or h["bad_flag"], sw                           # the word is -1 or the kernels write it
        seen.add((mode, bool(h["done_flag"]), bool(h["bad_flag"]), bool(h["fill_x"]), unknown))
    # the asymmetry the decision keeps: without a device prior the fused epilogue counts, the launch of its own does not
    base = dict(host_direct=1, p_xT=0, lik_x=0, prior=0, prior_rows=0, h_done=1, done_ticket=1, h_clean=1, clean_count=1,
                fill_rejected=1, h_x=1)
    fused, own = query(lib, dict(base, epilogue=1)), query(lib, dict(base, epilogue=0))
    assert fused[0]["bad_flag"] == ADDR["h_clean"] and fused[0]["fill_x"] == ADDR["cur_x"] and fused[2] == 0
    assert (own[0]["bad_count"], own[0]["bad_flag"], own[0]["fill_x"], own[2]) == (0, 0, 0, 1)
    assert len(seen) >= 8


def test_the_query_refuses_null_arguments(lib):
    from pocomc_amd import _lib
    h, m, u = _lib.pmc_handover_t(), C.c_int32(), C.c_int32()
    assert lib.pmc_step_handover(None, 0, 0, C.byref(h), C.byref(m), C.byref(u)) != 0
    s = descriptor(dict.fromkeys(SWITCHES, 0))
    assert lib.pmc_step_handover(C.byref(s), 0, 0, None, C.byref(m), C.byref(u)) != 0
