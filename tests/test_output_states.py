"""The state rules of the optional outputs, as one table over all of them.

The per-feature tests each check their own switch; test_ctx_lifecycle.py walks the entry points but none of these
outputs.  Here one context goes through every state in which a fetch of an optional output can be asked for, and in
every state every one of the ten fetches is called: it either fails with DAGCON_ERR_STATE and its full message, or returns
what the same call returns on a context of its own.

The expected table is REQUIRES below, written by hand from the rules of include/dagcon.h: a fetch is valid after a
dagcon_fetch of a run whose upload was made with everything the fetch requires, and in no other state.  The cells in
which the library does something the header does not spell out are marked NOTE where they are checked:
  * dagcon_fetch_positions keeps returning the positions of the last fetch after a run that has not been fetched yet
    (the header says "before a fetch"; the host copy stays readable until the next fetch or upload replaces it);
  * a dagcon_upload_haps refused for its state leaves the results of the batch as they were (it is no failed upload)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = -8
MIN_COV, MIN_LEN, TRIM = 3, 30, 5
PILE = (2, 200000)

FETCHES = ("edits", "edit_support", "positions", "pileup_sites", "pileup", "site_reads", "site_alleles", "hap_tally",
           "window_phase", "hap_map")
# what the upload must have been made with for the fetch to be valid after dagcon_fetch ("records": a record upload,
# "windows": one with windows, "phase": dagcon_set_site_reads with phase != 0; the others: the switch of that name).
# hap_map is valid from dagcon_upload_haps to the next upload and never otherwise.
REQUIRES = {
    "edits": {"records", "edits"},
    "edit_support": {"records", "edits", "evid"},
    "positions": set(),
    "pileup_sites": {"pile"},
    "pileup": {"pile"},
    "site_reads": {"pile", "sr"},
    "site_alleles": {"pile", "sr", "al"},
    "hap_tally": {"pile", "sr", "phase", "hap"},
    "window_phase": {"pile", "sr", "phase", "wl", "windows", "records"},
}
ALL_ON = frozenset({"records", "windows", "edits", "evid", "pile", "sr", "phase", "al", "hap", "wl"})
# the walk of a fetch is made with what it requires and nothing else (a record upload in every case)
CONFIGS = {f: frozenset(REQUIRES[f] | {"records"}) for f in REQUIRES}
CONFIGS["positions"] = frozenset({"records", "edits"})               # (edits on: the positions come when asked for)
CONFIGS["hap_map"] = CONFIGS["hap_tally"]

_PILE_STATE = ("without the results of an upload made with dagcon_set_pileup on (switch off at the upload, no fetch yet, or stopped "
               "before bestPath)")
_HAP_STATE = ("without the results of an upload made with dagcon_set_pileup, dagcon_set_site_reads (phase on) and "
              "dagcon_set_hap_consensus on (a switch off at the upload, no fetch yet, stopped before bestPath, or the batch is "
              "dagcon_upload_haps' own)")
TEXT = {
    "edits": "dagcon_fetch_edits without the results of a record upload made with dagcon_set_edits on (edits off, another kind of "
             "upload, no fetch yet, or stopped before bestPath)",
    "edit_support": "dagcon_fetch_edit_support without the results of a record upload made with dagcon_set_edit_support on (switch "
                    "off at the upload, edits off, another kind of upload, no fetch yet, or stopped before bestPath)",
    "positions": "dagcon_fetch_positions without the results of a consensus (no fetch yet, or stopped before bestPath)",
    "pileup_sites": "dagcon_fetch_pileup_sites " + _PILE_STATE,
    "pileup": "dagcon_fetch_pileup " + _PILE_STATE,
    "site_reads": "dagcon_fetch_site_reads without the results of an upload made with dagcon_set_pileup and dagcon_set_site_reads "
                  "on (a switch off at the upload, no fetch yet, or stopped before bestPath)",
    "site_alleles": "dagcon_fetch_site_alleles without the results of an upload made with dagcon_set_pileup, dagcon_set_site_reads "
                    "and dagcon_set_site_alleles on (a switch off at the upload, no fetch yet, or stopped before bestPath)",
    "hap_tally": "dagcon_fetch_hap_tally " + _HAP_STATE,
    "window_phase": "dagcon_fetch_window_phase without the results of a windows upload made with dagcon_set_pileup, "
                    "dagcon_set_site_reads (phase on) and dagcon_set_window_phase on (a switch off at the upload, no windows, no "
                    "fetch yet, or stopped before bestPath)",
    "hap_map": "dagcon_fetch_hap_map without a dagcon_upload_haps as the last upload",
    "upload_haps": "dagcon_upload_haps " + _HAP_STATE,
}


def _valid(cfg):
    """The fetches REQUIRES allows after a dagcon_fetch of an upload made under cfg."""
    return {f for f, need in REQUIRES.items() if need <= cfg}


# ---- the input ------------------------------------------------------------------------------------------------------

def make_data():
    """Two targets of 120 bases and 12 reads each, all of them from end to end.  Every read differs from its target at
    positions 10 and 110 (so the consensus does, and edits exist); reads 0-5 carry another base than reads 6-11 at
    positions 45 and 70 (two heterozygous sites, inside both windows of the target); read 1 has a 2-base insertion
    and read 7 a deletion.  The same records as a CIGAR batch and as windows of width 60, overlap 20; and a batch of
    strings for the uploads that are no record uploads."""
    from pbdagcon_amd import capi, synth
    rng = np.random.default_rng(11)
    nxt = bytes.maketrans(b"ACGT", b"CGTA")
    targets = []
    for _ in range(2):
        tgt = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 120).tolist())
        base = bytearray(tgt)
        for x in (10, 110):
            base[x:x + 1] = base[x:x + 1].translate(nxt)
        recs = []
        for r in range(12):
            q = bytearray(base)
            if r < 6:
                for x in (45, 70):
                    q[x:x + 1] = q[x:x + 1].translate(nxt)
            if r == 1:
                recs.append((1, bytes(q[:20] + b"GT" + q[20:]), [("M", 20), ("I", 2), ("M", 100)]))
            elif r == 7:
                recs.append((1, bytes(q[:100] + q[101:]), [("M", 100), ("D", 1), ("M", 19)]))
            else:
                recs.append((1, bytes(q), [("M", 120)]))
        targets.append((tgt, recs))
    return {"cigar": capi.HostCigarBatch.from_records(targets), "windows": capi.HostWindows.tiled([120, 120], 60, 20),
            "strings": synth.make_batch(2, 200, 8, seed=1)}


@pytest.fixture(scope="module")
def data():
    return make_data()


def _ctx():
    from pbdagcon_amd import capi
    return capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS)


def _set(ctx, cfg):
    ctx.set_edits("edits" in cfg)
    if "edits" in cfg:
        ctx.set_edit_support("evid" in cfg)                          # (turning edits off has turned it off)
    ctx.set_pileup(*PILE) if "pile" in cfg else ctx.set_pileup(None)
    ctx.set_site_reads("phase" in cfg) if "sr" in cfg else ctx.set_site_reads(None)
    ctx.set_site_alleles("al" in cfg)
    ctx.set_hap_consensus() if "hap" in cfg else ctx.set_hap_consensus(None)
    ctx.set_window_phase() if "wl" in cfg else ctx.set_window_phase(None)


def _upload(ctx, data, cfg, consensus):
    """The upload of cfg's kind, or the consensus call of that kind (upload, run and fetch in one)."""
    if "windows" in cfg:
        f = ctx.consensus_cigar_windows if consensus else ctx.upload_cigar_windows
        return f(data["cigar"], data["windows"])
    if "records" in cfg:
        return (ctx.consensus_cigar if consensus else ctx.upload_cigar)(data["cigar"])
    return (ctx.consensus if consensus else ctx.upload)(data["strings"])


def _get(ctx, name):
    """What a fetch returns, in a form that does not depend on where a target lies in seq_blob."""
    if name == "positions":
        return [[p.tobytes() for p in segs] for segs in ctx.base_positions()]
    out = dict(getattr(ctx, name)())
    if name == "edits":
        so = ctx._segs[1].astype(np.int64)
        out["c_off"] = out["c_off"].astype(np.int64) - np.repeat(so, np.diff(out["edit_begin"].astype(np.int64)))
    return {k: None if v is None else (v.dtype.str, v.shape, v.tobytes()) for k, v in out.items()}


_REF = {}


def _ref(data, cfg):
    """Every valid fetch of a consensus made under cfg on a context of its own, and the hap map that follows it."""
    if cfg not in _REF:
        ctx = _ctx()
        try:
            _set(ctx, cfg)
            _upload(ctx, data, cfg, True)
            ref = {f: _get(ctx, f) for f in FETCHES if f in _valid(cfg)}
            if "hap_tally" in ref:
                ctx.upload_haps()
                ref["hap_map"] = _get(ctx, "hap_map")
            _REF[cfg] = ref
        finally:
            ctx.close()
    return _REF[cfg]


def _check(ctx, want, order, where, skip=()):
    """Every fetch in `order`: the arrays of `want`, or DAGCON_ERR_STATE with the fetch's own text."""
    from pbdagcon_amd import capi
    for f in order:
        if f in skip:
            continue
        if f in want:
            assert _get(ctx, f) == want[f], (where, f)
        else:
            with pytest.raises(capi.DagconError) as e:
                _get(ctx, f)
            assert e.value.code == STATE and str(e.value) == "DAGCON_ERR_STATE: " + TEXT[f], (where, f)


def _pick(ref, names):
    return {f: ref[f] for f in names if f in ref}


def _refused_upload(ctx, data):
    """n_targets > 0 with a NULL tlen: the first thing dagcon_upload refuses, after it has dropped the results."""
    b = data["strings"].c_struct()
    b.tlen = None
    assert ctx.L.dagcon_upload(ctx.h, C.byref(b)) == -1
    assert ctx.L.dagcon_last_error(ctx.h) == b"tlen/aln_begin is NULL"


def _refused_record_upload(ctx, data):
    """The same through the record intake, which resets the context on its own before it checks anything."""
    b = data["cigar"].c_struct()
    b.tlen = None
    assert ctx.L.dagcon_upload_cigar(ctx.h, C.byref(b)) == -1
    assert ctx.L.dagcon_last_error(ctx.h) == b"tlen/t_off/rec_begin is NULL"


def _walk(data, cfg, order):
    from pbdagcon_amd import capi
    ref = _ref(data, cfg)
    fetchable = _valid(cfg)
    off = frozenset({"records"})
    ctx = _ctx()
    try:
        _check(ctx, {}, order, "before any upload")
        # the output's own switch off, or a prerequisite off: one state for each thing the upload was made with
        for r in sorted(cfg):
            if r == "records" and "windows" in cfg:
                continue                                             # (windows without records: no such upload)
            less = frozenset(cfg - {r} - ({"phase"} if r == "sr" else set()) - ({"evid"} if r == "edits" else set()))
            _set(ctx, less)
            _upload(ctx, data, less, True)
            _check(ctx, _pick(_ref(data, less), _valid(less)), order, ("without", r))
        _set(ctx, cfg)
        _upload(ctx, data, cfg, False)
        _check(ctx, {}, order, "after an upload")
        ctx.run(); ctx.sync()
        _check(ctx, {}, order, "after a run without a fetch")
        ctx.fetch()
        _check(ctx, _pick(ref, fetchable), order, "after a fetch")
        _check(ctx, _pick(ref, fetchable), order, "the same fetches again")
        ctx.fetch()
        _check(ctx, _pick(ref, fetchable), order, "after a second fetch of the same run")
        ctx.run(); ctx.sync()
        # NOTE: the positions of the last fetch stay readable (a run drops everything else)
        _check(ctx, _pick(ref, {"positions"}), order, "after a second run without a fetch")
        _upload(ctx, data, cfg, True)
        _check(ctx, _pick(ref, fetchable), order, "after a full consensus call")
        if "hap_tally" in fetchable:
            ctx.upload_haps()
            _check(ctx, _pick(ref, {"hap_map"}), order, "after dagcon_upload_haps")
            with pytest.raises(capi.DagconError) as e:
                ctx.upload_haps()
            assert e.value.code == STATE and str(e.value) == "DAGCON_ERR_STATE: " + TEXT["upload_haps"]
            ctx.run(); ctx.sync(); ctx.fetch()
            _check(ctx, _pick(ref, {"hap_map"}), order, "after the fetch of the derived batch", skip=("positions",))
        else:
            with pytest.raises(capi.DagconError) as e:
                ctx.upload_haps()
            assert e.value.code == STATE and str(e.value) == "DAGCON_ERR_STATE: " + TEXT["upload_haps"]
            # NOTE: refused for its state, it has touched nothing
            _check(ctx, _pick(ref, fetchable), order, "after a refused dagcon_upload_haps")
        _set(ctx, off)
        _upload(ctx, data, off, True)
        _check(ctx, _pick(_ref(data, off), {"positions"}), order, "after a new upload with everything off")
        _set(ctx, cfg)
        _upload(ctx, data, cfg, True)
        _check(ctx, _pick(ref, fetchable), order, "switched on again")
        _refused_upload(ctx, data)
        _check(ctx, {}, order, "after an upload that failed")
        _upload(ctx, data, cfg, True)
        _check(ctx, _pick(ref, fetchable), order, "after the upload that followed it")
        _refused_record_upload(ctx, data)
        _check(ctx, {}, order, "after a record upload that failed")
    finally:
        ctx.close()


def test_the_input_gives_every_output_something(data):
    ref = _ref(data, ALL_ON)
    assert set(ref) == set(FETCHES)
    n = {f: {k: (np.frombuffer(v[2], v[0]).reshape(v[1]) if v is not None else None) for k, v in ref[f].items()}
         for f in FETCHES if f != "positions"}
    assert n["edits"]["t_pos"].size > 0 and n["edit_support"]["alt"].size == n["edits"]["t_pos"].size
    assert n["pileup_sites"]["pos"].size >= 4 and n["site_reads"]["hap"].any() and n["site_alleles"]["key"].size > 0
    assert n["hap_tally"]["split"].any() and n["hap_map"]["label"].size > 0
    assert (n["window_phase"]["block"] != np.arange(4)).any()       # (windows were joined)
    whole = _ref(data, frozenset(ALL_ON - {"windows", "wl"}))
    assert np.frombuffer(whole["hap_tally"]["split"][2], np.uint8).all()


@pytest.mark.parametrize("fetch", FETCHES)
def test_states_of(data, fetch):
    _walk(data, CONFIGS[fetch], FETCHES)


def test_states_with_every_switch_on(data):
    _walk(data, ALL_ON, FETCHES)


def test_states_with_the_outer_fetches_first(data):
    """dagcon_fetch_site_alleles and dagcon_fetch_window_phase call dagcon_fetch_site_reads themselves: here they come
    before it, in every state."""
    first = ("site_alleles", "window_phase", "site_reads")
    _walk(data, ALL_ON, first + tuple(f for f in FETCHES if f not in first))
