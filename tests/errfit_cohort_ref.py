"""Numpy restatement of the POOLED error-rate fit of a cohort (vb2_abi.h section 3h), on top of
tests/errfit_ref.py: one error table for all samples, written here as plain Python over the restatement's log-likelihood
and E-step -- its own loop, its own M-step, its own stop rule -- so that the library's statement of the procedure
(errfit_cohort.cpp, reached without a device through vb2_errfit_cohort_lockstep) has something to be held against.

    start      eps_0 the nominal table; every sample at its own nominal estimate
    iteration  (n_s, s_s) of every sample still in at (est_s,t, eps_t); N = sum n_s in integers, SUM = the s_s added in
               list order; eps_{t+1}[q] = float32((SUM[q] + kappa eps0[q]) / (N[q] + kappa)) where N[q] > 0, else eps0[q]
               (kappa is not scaled by the number of samples); then every sample's search under eps_{t+1}
    stop       after the iteration whose largest relative change over N[q] > 0 is within tol, else after max_iter
    report     one more E-step at the final (est_s, eps)

The searches are the library's host optimiser over the restatement's evaluator (vb.optimize_with_evaluator), as in
errfit_ref.Evaluator: the reference-exact OptimizeLLK from the reference's start.
"""
import numpy as np

import errfit_ref as er
import verifybamid_amd as vb

Q = er.NUM_QUAL


def search_point(est, known_af, within_ancestry=False):
    """The search's own point of an estimate: the reference's swap of PC indices 0, 1 for alpha >= 0.5 undone."""
    p1, p2 = np.array(est["pc"], dtype=np.float64), np.array(est["pc2"], dtype=np.float64)
    if not within_ancestry and not known_af and est["alpha"] >= 0.5:
        for j in range(min(2, len(p1))):
            p1[j], p2[j] = p2[j], p1[j]
    return p1, p2


def mstep(N, S, eps, kappa):
    """(eps_{t+1}, the stop rule's maximum)."""
    e0 = vb.nominal_err_table()
    nxt = e0.copy()
    has = N > 0
    nxt[has] = ((S[has] + kappa * e0[has]) / (N[has].astype(np.float64) + kappa)).astype(np.float32).astype(np.float64)
    change = 0.0
    for q in np.nonzero(has)[0]:
        d = abs(nxt[q] - eps[q]) / eps[q] if eps[q] > 0 else (0.0 if nxt[q] == 0 else np.inf)
        change = max(change, d)
    return nxt, change


def unrounded_mstep(N, S, kappa):
    """The M-step's values before the float32 rounding, where N > 0 (for the check that none sits on a rounding boundary)."""
    e0 = vb.nominal_err_table()
    has = N > 0
    return (S[has] + kappa * e0[has]) / (N[has].astype(np.float64) + kappa)


def log_prior(eps, kappa):
    """The Beta prior's logarithm, kappa pseudo-reads centred on the nominal rate of every quality (up to a constant)."""
    e0 = vb.nominal_err_table()
    with np.errstate(divide="ignore", invalid="ignore"):
        t = kappa * e0 * np.log(eps) + kappa * (1.0 - e0) * np.log1p(-eps)
    return float(np.sum(np.where(np.isfinite(t), t, 0.0)))


class Cohort:
    """Evaluators of the samples (errfit_ref.Evaluator) and the pooled procedure over them."""

    def __init__(self, datas, dtype=np.float64):
        self.ev = [None if d is None else er.Evaluator(d, dtype) for d in datas]
        held = [d for d in datas if d is not None]
        self.num_pc = held[0].num_pc
        self.known_af = held[0].known_af is not None

    def nominal_estimates(self, **model_kw):
        return [None if ev is None else ev.nominal_estimate(self.num_pc, self.known_af, **model_kw) for ev in self.ev]

    # the two callbacks of vb.errfit_cohort_with_evaluator
    def eval(self, sample, err, pc1, pc2, alpha):
        return self.ev[sample].eval(err, pc1, pc2, alpha)

    def stats(self, live, err, pc1, pc2, alpha):
        n, s = np.zeros((len(self.ev), Q), dtype=np.int64), np.zeros((len(self.ev), Q))
        for i in np.nonzero(live)[0]:
            n[i], s[i] = self.ev[i].stats(err[i], pc1[i], pc2[i], alpha[i])
        return n, s

    def search(self, i, table, **model_kw):
        return vb.optimize_with_evaluator(lambda a, b, al: self.ev[i].eval(table, a, b, al), self.num_pc, known_af=self.known_af,
                                          **model_kw)

    def pooled_fit(self, nominals, enter_status=None, prior_reads=100.0, tol=1e-4, max_iter=24, **model_kw):
        """(fits, pool) in the shape of vb.errfit_cohort; pool["unrounded"]: every iteration's M-step values before the
        rounding; pool["iter_logpost"]: the pooled log-posterior after every iteration."""
        S = len(self.ev)
        within = bool(model_kw.get("within_ancestry", False))
        enter = np.zeros(S, dtype=np.int64) if enter_status is None else np.asarray(enter_status)
        inside = [i for i in range(S) if enter[i] == 0]
        status = {i: int(enter[i]) for i in range(S)}
        est = {i: dict(nominals[i]) for i in inside}
        e0 = vb.nominal_err_table()
        eps = e0.copy()
        rec = {i: dict(iter_llk=[], iter_alpha=[], num_step=0) for i in inside}
        tables, changes, unrounded, logpost = [], [], [], []
        converged = False

        def estep(who, table):
            out = {}
            for i in who:
                p1, p2 = search_point(est[i], self.known_af, within)
                out[i] = self.ev[i].stats(table, p1, p2, est[i]["alpha"])
            return out

        for _ in range(max_iter):
            if not inside:
                break
            st = estep(inside, eps)
            N, SUM = np.zeros(Q, dtype=np.int64), np.zeros(Q)
            for i in inside:                            # list order
                N += st[i][0]
                SUM += st[i][1]
            unrounded.append(unrounded_mstep(N, SUM, prior_reads))
            nxt, change = mstep(N, SUM, eps, prior_reads)
            for i in list(inside):
                try:
                    est[i] = self.search(i, nxt, **model_kw)
                except (vb._abi.Vb2Error, vb.SearchFailed) as exc:          # the sample leaves with its code
                    status[i] = exc.code
                    inside.remove(i)
                    continue
                rec[i]["iter_llk"].append(-est[i]["llk1"])
                rec[i]["iter_alpha"].append(est[i]["alpha"])
                rec[i]["num_step"] += est[i]["num_eval"]
            eps = nxt
            tables.append(eps.astype(np.float32))
            changes.append(change)
            logpost.append(sum(rec[i]["iter_llk"][-1] for i in inside) + log_prior(eps, prior_reads))
            if change <= tol:
                converged = True
                break
        final = estep(inside, eps)
        fits = []
        T = len(tables)
        for i in range(S):
            if i not in inside:
                fits.append(dict(status=status[i], num_iter=len(rec[i]["iter_llk"]) if i in rec else 0))
                continue
            n, s = final[i]
            llk_fit, llk_nom = -est[i]["llk1"], -nominals[i]["llk1"]
            fits.append(dict(err=eps.copy(), n=n, s=s, estimate=est[i], alpha_fit=est[i]["alpha"],
                             freemix_fit=min(est[i]["alpha"], 1 - est[i]["alpha"]), llk_fit=llk_fit, llk_nominal=llk_nom,
                             alpha_nominal=nominals[i]["alpha"], lrt=2.0 * (llk_fit - llk_nom), num_bin=int(np.sum(n > 0)),
                             num_iter=T, converged=converged, num_step=rec[i]["num_step"], status=0,
                             iter_llk=np.array(rec[i]["iter_llk"]), iter_change=np.array(changes),
                             iter_alpha=np.array(rec[i]["iter_alpha"]), iter_err=np.array(tables, dtype=np.float32).reshape(T, Q)))
        N, SUM = np.zeros(Q, dtype=np.int64), np.zeros(Q)
        for i in inside:
            N += final[i][0]
            SUM += final[i][1]
        pool = dict(err=eps.copy(), n=N, s=SUM, lrt_sum=float(sum(fits[i]["lrt"] for i in inside)), num_bin=int(np.sum(N > 0)),
                    num_iter=T, converged=converged, pooled=True, num_sample=S, num_entered=int(np.sum(enter == 0)),
                    num_fitted=len(inside), num_estep=T + (1 if inside else 0), num_step=sum(rec[i]["num_step"] for i in rec),
                    iter_change=np.array(changes), iter_err=np.array(tables, dtype=np.float32).reshape(T, Q),
                    unrounded=unrounded, iter_logpost=np.array(logpost))
        return fits, pool
