"""The inputs of the deny-mask kernel tests (tests/test_suppress_ref.py on the CPU, tests/test_gpu_suppress_kernels.py on
the device): per vocabulary a pool of logits rows with their SeqCtl, and 8 masks built from the pool. A mask is one per
launch, so a case is (mask, the first 17 pool rows that the float64 reference decides under that mask); nothing here
looks at a kernel.

The pool, rows at temperatures 0 / 0.2 / 1.0 in turn (t > 0 rows with want_probs), N(0, 6^2) like logits_cases' "unit"
rows: the maximum planted at each of the 11 seam ids (0, 31, 32: the first words of the mask; cs - 1, cs: the split
form's chunk, cs = ceil(V / 16); 36 * 1024 - 1, 36 * 1024: the LDS / register seam; eot - 1, eot, beg, V - 1), an initial
row without suppress_blank whose maximum is eot, a row whose timestamp mass sits 4e-3 nats below its best text token
(logits_cases._mass_row), random rows in several rule states, and spares that take the place of rows a mask leaves
undecided.

A row is kept under a mask when every decision of the reference has a gap of at least logits_cases.MIN_GAP (top2_gap,
ts_gap, tid_gap: logits_cases._decided, as test_logits_ref.py holds its own rows).
"""
import numpy as np

import logits_cases as lc
import suppress_ref as sr

N_ROWS = 17
MASKS = ("argmax", "best text", "best timestamp", "all text", "everything", "eot", "empty", "random 1%")
K_TOP = 5


def seams(V: int, v: dict) -> list:
    cs = (V + 15) // 16
    return [0, 31, 32, cs - 1, cs, 36 * 1024 - 1, 36 * 1024, v["eot"] - 1, v["eot"], v["beg"], V - 1]


def _with_temp(c: dict, t: float) -> dict:
    c = dict(c)
    c.update(temperature=t, want_probs=int(t > 0))
    return c


def build_pool(V: int) -> list:
    v = lc.vocab(V)
    st = dict(lc.states())
    text = st["text,text"]
    rows = []

    def add(make, c, what, **kw):
        r = len(rows)
        t = lc.TEMPS[r % 3]
        c = _with_temp(c, t)
        if r % 5 == 3:
            c["want_nosp"] = 1
        rows.append(lc._row(V, v, lambda rng: make(rng, c, t), c, 700000 + 17 * r + V % 7, what, **kw))

    def planted(idx):
        def make(rng, c, t):
            x = rng.normal(0.0, 6.0, V)
            x[idx] = x.max() + 5.0
            return x
        return make

    for idx in seams(V, v):
        add(planted(idx), text, f"max at {idx}", expect=dict(id=idx))
    add(planted(v["eot"]), dict(st["initial"]), "initial, max at eot", expect=dict(id=v["eot"]))
    add(lambda rng, c, t: lc._mass_row(rng, V, v, c, -1, t), text, "mass below", expect=dict(ts_fired=False, id=1000))
    for name in ("initial+blank", "text,ts", "has_ts 20", "ts,ts", "text,text", "has_ts 2998", "suppress_eot", "initial",
                 "text,text", "has_ts 21", "text,text"):
        add(lambda rng, c, t: rng.normal(0.0, 6.0, V), st[name], f"random, {name}")
    return rows


def build_masks(V: int, pool: list) -> dict:
    v = lc.vocab(V)
    beg, eot = v["beg"], v["eot"]
    sm = seams(V, v)
    m = {k: np.zeros(V, bool) for k in MASKS}
    for row in pool:
        ref = row["ref"]
        if ref["p"] > 0:
            m["argmax"][ref["id"]] = True
            lp = ref["logprobs"]
            # the best text token before the timestamp rule struck it: from the filtered logits
            x = sr.lr.masked(row["raw"], row["ctl"], v)
            if np.isfinite(x[:beg]).any():
                m["best text"][int(np.argmax(x[:beg]))] = True
            if np.isfinite(lp[beg:]).any():
                m["best timestamp"][beg + int(np.argmax(lp[beg:]))] = True
    m["all text"][:eot] = True
    m["everything"][:] = True
    m["eot"][eot] = True
    m["random 1%"] = np.random.default_rng(4242 + V).random(V) < 0.01
    for k in ("argmax", "best text", "best timestamp", "eot", "random 1%"):
        m[k][sm] = True
    return m


def decided(ref: dict) -> bool:
    return lc._decided(ref, None, lc.MIN_GAP)


_BUILT = {}


def cases(V: int) -> dict:
    """{mask name: dict(deny=bool [V], rows=[17 x dict(raw, ctl, ref, what, pool_index)])}, built once per vocabulary."""
    if V in _BUILT:
        return _BUILT[V]
    v = lc.vocab(V)
    pool = build_pool(V)
    out = {}
    for name, deny in build_masks(V, pool).items():
        rows = []
        for i, row in enumerate(pool):
            ref = sr.process(row["raw"], row["ctl"], v, deny)
            if decided(ref):
                rows.append(dict(raw=row["raw"], ctl=row["ctl"], ref=ref, what=row["what"], pool_index=i, plain=row["ref"]))
            if len(rows) == N_ROWS:
                break
        assert len(rows) == N_ROWS, f"{V} {name}: {len(rows)} decided rows"
        out[name] = dict(deny=deny, rows=rows)
    _BUILT[V] = out
    return out


def topk_decided(lp: np.ndarray, ref: dict, k: int) -> bool:
    """The k candidates and their order are decided: successive gaps among the k + 1 largest logprobs, and the rule."""
    top = np.sort(lp[np.isfinite(lp)])[::-1][:k + 1]
    return decided(ref) and (top.size < 2 or float(np.min(top[:-1] - top[1:])) >= lc.MIN_GAP)


_TOPK = {}


def topk_cases(V: int) -> dict:
    """{name: dict(deny, rows)}: 16 pool rows at temperature 0 under the random 1 % mask, and under a mask that leaves
    3 tokens (a text token, eot and a timestamp); rows whose k + 1 best are undecided are left out of the comparison
    (row["check"] = False), not of the launch."""
    if V in _TOPK:
        return _TOPK[V]
    v = lc.vocab(V)
    pool = build_pool(V)[:16]
    masks = build_masks(V, pool)
    three = np.ones(V, bool)
    three[[4242, v["eot"], v["beg"] + 700]] = False
    out = {}
    for name, deny in (("random 1%", masks["random 1%"]), ("3 tokens left", three)):
        rows = []
        for row in pool:
            c = _with_temp(row["ctl"], 0.0)
            ref = sr.process(row["raw"], c, v, deny)
            rows.append(dict(raw=row["raw"], ctl=c, ref=ref, what=row["what"], check=topk_decided(ref["logprobs"], ref, K_TOP)))
        out[name] = dict(deny=deny, rows=rows)
    _TOPK[V] = out
    return out
