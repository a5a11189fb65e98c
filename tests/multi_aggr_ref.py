"""Plain numpy float64 restatement of spmm_multi (paddle_sparse_amd/multi_aggr.py): per row the messages
m_e = value[e] * x[col[e]], the six statistics, the first winner of min / max, and the gradient wrt x."""
import numpy as np

NAMES = ("sum", "mean", "min", "max", "var", "std")


def forward(rowptr, col, value, x, reduce, eps):
    """out [M, A, K] float64, {"min": arg_min, "max": arg_max} int64 [M, K] (nnz: no entry), and
    ex2 [M, K] = sum of m^2 / n (0 for a row without entries), which scales the var / std tolerances."""
    rowptr, col, x = np.asarray(rowptr), np.asarray(col), np.asarray(x, dtype=np.float64)
    M, K, nnz = len(rowptr) - 1, x.shape[1], len(col)
    v = np.ones(nnz) if value is None else np.asarray(value, dtype=np.float64)
    stat = {n: np.zeros((M, K)) for n in NAMES}
    arg = {n: np.full((M, K), nnz, dtype=np.int64) for n in ("min", "max")}
    ex2 = np.zeros((M, K))
    for i in range(M):
        s, e = rowptr[i], rowptr[i + 1]
        if e == s:
            continue  # a row without entries is 0 in every statistic
        m = v[s:e, None] * x[col[s:e]]
        stat["sum"][i], stat["mean"][i] = m.sum(0), m.sum(0) / (e - s)
        stat["min"][i], stat["max"][i] = m.min(0), m.max(0)
        arg["min"][i], arg["max"][i] = s + m.argmin(0), s + m.argmax(0)  # the first one on ties
        ex2[i] = (m * m).sum(0) / (e - s)
        stat["var"][i] = np.maximum(ex2[i] - stat["mean"][i] ** 2, 0.0)
        stat["std"][i] = np.sqrt(stat["var"][i] + eps)
    out = np.stack([stat["sum" if n == "add" else n] for n in reduce], axis=1)
    return out, arg, ex2


def grad_x(rowptr, col, value, x, reduce, eps, g, std_rel_err=None):
    """Gradient wrt x of sum(out * g), g [M, A, K]:
        grad_x = A^T (g_s + g_m / n - 2 gv mu / n) + x * ((A o A)^T (2 gv / n)) + [min / max: all of it to the
        first winner],  gv = g_v + g_d / (2 std).
    Also, per element of x: `terms` [N] (stored entries of the column), `largest` [N, K] (largest sum of the
    absolute pieces of one entry's term) and `slack` [N, K] (sum over the entries of |std piece| * std_rel_err[row],
    what a relative error of the forward's std does to the result; 0 without std_rel_err)."""
    rowptr, col, x, g = np.asarray(rowptr), np.asarray(col), np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    M, (N, K), nnz = len(rowptr) - 1, x.shape, len(col)
    v = np.ones(nnz) if value is None else np.asarray(value, dtype=np.float64)
    out, arg, _ = forward(rowptr, col, value, x, NAMES, eps)
    mu, std = out[:, 1], out[:, 5]
    at = {("sum" if n == "add" else n): a for a, n in enumerate(reduce)}
    gs = {n: (g[:, at[n]] if n in at else np.zeros((M, K))) for n in NAMES}
    grad, largest, slack, terms = np.zeros((N, K)), np.zeros((N, K)), np.zeros((N, K)), np.zeros(N, dtype=np.int64)
    for i in range(M):
        s, e = rowptr[i], rowptr[i + 1]
        n = e - s
        for p in range(s, e):
            j = col[p]
            gd = gs["std"][i] / (2.0 * std[i])
            lin = gs["sum"][i] + gs["mean"][i] / n
            pieces = [v[p] * lin, (gs["var"][i]) * (2.0 / n) * v[p] * (v[p] * x[j] - mu[i]),
                      gd * (2.0 / n) * v[p] * (v[p] * x[j] - mu[i]),
                      v[p] * gs["min"][i] * (arg["min"][i] == p), v[p] * gs["max"][i] * (arg["max"][i] == p)]
            grad[j] += sum(pieces)
            mag = (np.abs(v[p]) * (np.abs(gs["sum"][i]) + np.abs(gs["mean"][i]) / n)
                   + (np.abs(gs["var"][i]) + np.abs(gd)) * (2.0 / n) * np.abs(v[p]) * (np.abs(v[p] * x[j]) + np.abs(mu[i]))
                   + np.abs(pieces[3]) + np.abs(pieces[4]))
            largest[j] = np.maximum(largest[j], mag)
            if std_rel_err is not None:
                slack[j] += np.abs(gd) * (2.0 / n) * np.abs(v[p]) * (np.abs(v[p] * x[j]) + np.abs(mu[i])) * std_rel_err[i]
            terms[j] += 1
    return grad, terms, largest, slack
