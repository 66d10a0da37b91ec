"""Float64 reference of the logits rules with the grammar's penalty: logits_ref.process / suppress_ref.process
extended, not edited. The grammar rule runs after the timestamp rule and only when that rule did not mask the text
tokens: every token <= eot whose bit is set in the row's reject mask loses `penalty` from its filtered logit (-inf stays
-inf), the log-softmax is taken again, and id / p / plog / tid / pt / ptsum / probs / logprobs come from the second one.
The timestamp rule is not asked again."""
import math

import numpy as np

import logits_ref as lr
import suppress_ref as sr


def process(raw, c: dict, v: dict, deny=None, gram=None, penalty=0.0) -> dict:
    """gram: bool [V] (the row's reject mask; bits above eot are ignored) or None = no grammar. The result has
    logits_ref.process's keys, and gram_applied."""
    raw = np.asarray(raw, np.float32)
    V, beg, eot = v["n_vocab"], v["beg"], v["eot"]
    deny = np.zeros(V, bool) if deny is None else np.asarray(deny, bool)
    first = sr.process(raw, c, v, deny)
    first["gram_applied"] = False
    if gram is None or first["ts_fired"] or not np.isfinite(first["logprobs"]).any():
        return first
    cut = raw.copy()
    cut[deny] = -np.inf
    x = lr.masked(cut, c, v)
    pen = np.asarray(gram, bool).copy()
    pen[eot + 1:] = False
    x[pen] -= float(np.float32(penalty))
    fin = np.isfinite(x)
    mx = x[fin].max()
    lse = math.log(np.exp(x[fin] - mx).sum()) + mx
    lp = np.where(fin, x - lse, -np.inf)
    p = np.exp(lp)
    out = dict(first)
    top = np.sort(lp[fin])[::-1]
    out["top2_gap"] = float(top[0] - top[1]) if top.size > 1 else math.inf
    i = int(np.argmax(lp))
    pts = p[beg:]
    sum_ts = float(pts.sum())
    tst = np.sort(lp[beg:][np.isfinite(lp[beg:])])[::-1]
    out["tid_gap"] = float(tst[0] - tst[1]) if tst.size > 1 else math.inf
    tid = beg + int(np.argmax(pts)) if pts.size and np.float32(pts.max()) > 0 else 0
    pt = float(pts.max() / (sum_ts + 1e-10)) if pts.size else 0.0
    if i >= beg:
        tid, pt = i, float(p[i])
    out.update(logprobs=lp, probs=p, suppressed=~fin, id=i, tid=tid, p=float(p[i]), plog=float(lp[i]), pt=pt, ptsum=sum_ts,
               tid_lp=float(lp[beg:].max()) if pts.size else -math.inf, gram_applied=True)
    return out
