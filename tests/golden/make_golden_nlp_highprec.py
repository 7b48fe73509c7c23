"""Generator of fixture G16 (tests/golden/G16_nlp_highprec.npz): the node functions of the two min-time NLPs and their first
derivatives at 50 digits (mpmath; tests/nlp_highprec.py), on input families that reach every branch of the device's elementary
functions.  CPU only:  python tests/golden/make_golden_nlp_highprec.py

Per double-track family F (tests/nlp_highprec.py: DT_FAMILIES):
  F_seed, F_s, F_kappa, F_left, F_right, F_L, F_margin, F_X [B,N,6], F_U [B,N,4], F_T [B,N]   the inputs of the entry points
  F_pairs [P,2]                            (instance, left node) of the stored pairs
  F_ref_val [P,23,2], F_ref_jac [P,23,21,2]   reference as double pairs (hi, lo): rows 0-7 eq, 8-21 ineq, 22 the pair's cost term
  F_twin_val [P,23], F_twin_jac [P,23,21]      the float twin and the float dual
  F_atan_kin [P,12], F_atan_pac [P,12], F_sincos [P,26]   arguments of the m_atan / m_sincos call sites (float twin)
  F_kinks [P,8]                            distances from the kinks (nlp_highprec.KINKS)
Per bicycle family (bk_sweep, bk_general): F_P0, F_yaw, F_X, F_U, F_T, F_ref [N,8,2], F_twin [N,8], F_sincos [N,8], F_atan [N,4],
F_yawdist [N].  Seeds are advanced until the kink conditions (every pair) and the coverage conditions (over all families) hold."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import nlp_highprec as hp  # noqa: E402

FIRST_SEED = {"tame": 1601, "cornering": 1602, "blend": 1603, "wraps": 1604, "limits": 1605, "shape": 1606}


def dt_family_arrays(name, model, fam, M, pairs=None):
    """Reference, twins and notes of the stored pairs (or of `pairs`, rows of fam['pairs']) of one family."""
    rows = fam["pairs"] if pairs is None else fam["pairs"][pairs]
    out = {k: [] for k in ("ref_val", "ref_jac", "twin_val", "twin_jac", "atan_kin", "atan_pac", "sincos", "kinks")}
    for b, j in rows:
        z, trk = hp.pair_inputs(fam, int(b), int(j))
        val, jac = hp.dt_reference(M, model, trk, z)
        tv, notes = hp.dt_float(model, trk, z, record=True)
        dv, dj = hp.dt_dual(model, trk, z)
        assert np.array_equal(tv, dv)
        out["ref_val"].append(val); out["ref_jac"].append(jac); out["twin_val"].append(tv); out["twin_jac"].append(dj)
        for k in ("atan_kin", "atan_pac", "sincos"):
            out[k].append(notes[k])
        out["kinks"].append(hp.kinks_of(notes))
    return {f"{name}_{k}": np.array(v) for k, v in out.items()}


def bk_family_arrays(name, model, fam, M, nodes=None):
    sel = range(len(fam["T"])) if nodes is None else nodes
    F = hp.FloatMath(record=True)
    twin = np.array(hp.bk_eval(F, model, fam))
    ref = hp.bk_eval(M, model, fam, conv=M.num)
    N = len(fam["T"])
    out = {f"{name}_ref": np.array([hp.hi_lo(M, ref[j]) for j in sel]), f"{name}_twin": twin[list(sel)],
           f"{name}_sincos": np.array(F.notes["sincos"]).reshape(N, 8)[list(sel)],
           f"{name}_atan": np.array(F.notes["atan_bk"]).reshape(N, 4)[list(sel)],
           f"{name}_yawdist": np.array(F.notes["yaw"])[list(sel)]}
    return out


def coverage_holds(arrays):
    kin = np.concatenate([arrays[f"{f}_atan_kin"] for f in hp.DT_FAMILIES])
    pac = np.concatenate([arrays[f"{f}_atan_pac"] for f in hp.DT_FAMILIES])
    sc = np.concatenate([arrays[f"{f}_sincos"].ravel() for f in hp.DT_FAMILIES + ("bk_sweep", "bk_general")])
    return hp.atan_coverage(kin).min() >= 3 and hp.atan_coverage(pac).min() >= 3 and hp.sincos_coverage(sc).min() >= 3


def main():
    from bicycle_problem import MODEL as BK_MODEL
    from test_double_track import MODEL
    M = hp.MpMath()
    arrays = {}
    for name in ("bk_sweep", "bk_general"):
        fam = hp.bk_sweep_family() if name == "bk_sweep" else hp.bk_general_family()
        arrays.update({f"{name}_{k}": v for k, v in fam.items()})
        arrays.update(bk_family_arrays(name, BK_MODEL, fam, M))
        assert arrays[f"{name}_yawdist"].min() >= 1e-3
        print(name, "done", flush=True)
    seeds = dict(FIRST_SEED)
    fams = {}
    while True:
        for name in hp.DT_FAMILIES:
            while name not in fams:
                fam = hp.draw_dt_family(name, MODEL, seeds[name])
                if fam is None:
                    seeds[name] += 10
                else:
                    fams[name] = fam
        # the coverage conditions need only the float twin's notes
        notes = {}
        for name, fam in fams.items():
            rec = [hp.dt_float(MODEL, *reversed(hp.pair_inputs(fam, int(b), int(j))), record=True)[1] for b, j in fam["pairs"]]
            for k in ("atan_kin", "atan_pac", "sincos"):
                notes[f"{name}_{k}"] = np.array([r[k] for r in rec])
        notes.update({k: arrays[k] for k in ("bk_sweep_sincos", "bk_general_sincos")})
        if coverage_holds(notes):
            break
        del fams["cornering"]
        seeds["cornering"] += 10
    for name, fam in fams.items():
        arrays[f"{name}_seed"] = np.int64(seeds[name])
        arrays.update({f"{name}_{k}": np.asarray(v) for k, v in fam.items()})
        arrays.update(dt_family_arrays(name, MODEL, fam, M))
        print(name, "seed", seeds[name], "pairs", len(fam["pairs"]), flush=True)
    path = os.path.join(HERE, "G16_nlp_highprec.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
