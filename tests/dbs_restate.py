"""List-level restatement of the reference's `diverse_beam_search` loop and result (models/gridTDmodel.py:337-392; the other four model
classes run the same lines on their own step) over a step function - no model, no device.  The arithmetic is fp32 in the reference's
order, `cum + ((x - lse) - diversity_prob)`; the selection is spelt out (descending score, ascending flat index), since a library top-k
promises no order among equal values.  tests/golden/make_golden_dbs.py checks it against the reference's own runs, the tests replay
recorded logits and drawn tables through it."""
import torch


def diverse_beam_search(step, V, beam_size, T, start, end, diversity_prob, log=None):
    """step(t, g, seqs) -> (len(seqs), V) scores of group g's live sequences at loop step t (their last tokens are the input words).
    Returns the reference's `seq` per group.  `log` (a dict) receives the events the goldens are chosen by and the smallest gap any
    selection rested on: between neighbouring kept candidates and to the first rejected one."""
    k = G = int(beam_size)
    seqs = [[[start] for _ in range(k)] for _ in range(G)]                 # :325
    cum = [torch.zeros(k) for _ in range(G)]                               # :324
    live = [k] * G                                                         # :336
    complete = [[] for _ in range(G)]                                      # :321-322 as (score, sequence)
    ev = dict(partial=False, passed_over=False, g0_done_g1_selects=False, fallback_after_g0_done=False, penalised_pick=False,
              min_gap=float("inf"), selections=0, g0_done_step=None)
    for t in range(T):
        previous = []                                                      # :338
        for g in range(G):
            if live[g] == 0:                                               # :340-341
                continue
            inputs = [s[-1] for s in seqs[g]]
            lp = torch.log_softmax(torch.as_tensor(step(t, g, seqs[g]), dtype=torch.float32).clone(), dim=-1)          # :345
            for v in previous:                                             # :346-347
                lp[:, v] = lp[:, v] - diversity_prob
            sc = cum[g][:live[g], None] + lp                               # :348-349
            flat, n = (sc[0], k) if t == 0 else (sc.reshape(-1), live[g])  # :350-353
            vals, order = torch.sort(flat, descending=True, stable=True)   # equal values: the lower flat index first
            top, tv = order[:n].tolist(), vals[:n]
            ev["selections"] += 1
            ev["min_gap"] = min(ev["min_gap"], float((vals[:n] - vals[1:n + 1]).min()) if len(vals) > n else float("inf"))
            ev["penalised_pick"] |= any(f % V in previous for f in top)
            ev["g0_done_g1_selects"] |= g == 1 and live[0] == 0
            cand = [seqs[g][f // V] + [f % V] for f in top]                # :354-357
            inc = [j for j, f in enumerate(top) if f % V != end]           # :358
            complete[g] += [(float(tv[j]), cand[j]) for j in range(n) if j not in inc]      # :359-363, ascending candidate index
            live[g] = len(inc)                                             # :364
            seqs[g] = cand
            if live[g] == 0:                                               # :365-366: the step ends here for the later groups too
                ev["passed_over"] |= any(live[h] > 0 for h in range(g + 1, G))
                if g == 0:
                    ev["g0_done_step"] = t
                break
            ev["partial"] |= len(inc) < n
            seqs[g] = [cand[j] for j in inc]                               # :368
            cum[g] = tv[inc]                                               # :376
            if g < 2:                                                      # :377-380
                for w in inputs:
                    if w not in previous:
                        previous.append(w)
    out = []
    for g in range(G):                                                     # :384-390
        if complete[g]:
            best = complete[g][0]
            for c in complete[g][1:]:
                if c[0] > best[0]:                                         # `index(max(...))`: the first maximum
                    best = c
            out.append(list(best[1]))
        else:
            ev["fallback_after_g0_done"] |= live[0] == 0
            out.append(list(seqs[0][0][:20]))
    if log is not None:
        log.update(ev)
    return out


def beam_search(step, V, beam_size, T, start, end):
    """the reference's `beam_search` (:433-473) in the same style: step(t, seqs) -> scores.  Group 0 of a diverse beam search is this."""
    k = int(beam_size)
    seqs, cum, live, complete = [[start] for _ in range(k)], torch.zeros(k), k, []
    for t in range(T):
        lp = torch.log_softmax(torch.as_tensor(step(t, seqs), dtype=torch.float32), dim=-1)
        sc = cum[:live, None] + lp
        flat, n = (sc[0], k) if t == 0 else (sc.reshape(-1), live)
        vals, order = torch.sort(flat, descending=True, stable=True)
        top, tv = order[:n].tolist(), vals[:n]
        cand = [seqs[f // V] + [f % V] for f in top]
        inc = [j for j, f in enumerate(top) if f % V != end]
        complete += [(float(tv[j]), cand[j]) for j in range(n) if j not in inc]
        live = len(inc)
        if live == 0:
            break
        seqs, cum = [cand[j] for j in inc], tv[inc]
    if complete:
        best = complete[0]
        for c in complete[1:]:
            if c[0] > best[0]:
                best = c
        return list(best[1])
    return list(seqs[0][:20])
