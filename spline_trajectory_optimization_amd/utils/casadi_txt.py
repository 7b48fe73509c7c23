"""Reader and writer of CasADi's dense "txt" matrix files (`DM.to_file(path, "txt")` / `DM.from_file(path, "txt")`), which
the reference's command-line tools use for the solver's initial guess and results (entrypoints/traj_opt_double_track.py,
traj_opt_convert_to_casadi.py).  CasADi is not a dependency of this package; these two functions are the part of it the
tools need.

Format: one matrix row per line, values separated by white space.  The writer prints every value with 17 significant digits
(a float64 survives the round trip bit for bit).  The reader also accepts `00` (CasADi's mark of a structural zero), `nan` /
`inf` in any letter case, and skips blank lines and lines that start with `%` or `#`.  A 1-D array is written as a column,
as casadi.DM makes a column vector of it."""
import numpy as np


def write_txt(path, values):
    """Write a scalar, vector (as a column) or matrix as CasADi "txt"."""
    a = np.asarray(values, dtype=np.float64)
    if a.ndim < 2:
        a = a.reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError(f"a CasADi matrix has two dimensions, got shape {a.shape}")
    with open(path, "w") as out:
        for row in a:
            out.write(" ".join(f"{v:.17g}" for v in row) + "\n")


def _value(token):
    return 0.0 if token == "00" else float(token)


def read_txt(path):
    """-> float64 array [rows, cols] of a CasADi "txt" file."""
    rows = []
    with open(path, "r") as src:
        for num, line in enumerate(src, 1):
            text = line.strip()
            if not text or text[0] in "%#":
                continue
            try:
                rows.append([_value(tok) for tok in text.split()])
            except ValueError as err:
                raise ValueError(f"{path}:{num}: not a CasADi txt row: {text!r}") from err
            if len(rows[-1]) != len(rows[0]):
                raise ValueError(f"{path}:{num}: {len(rows[-1])} values, the first row has {len(rows[0])}")
    return np.array(rows, dtype=np.float64).reshape(len(rows), len(rows[0]) if rows else 0)
