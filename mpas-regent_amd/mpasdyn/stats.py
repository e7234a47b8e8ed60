"""Host layer of the sigma-level statistics (include/mpas_dyn.h, mpas_atm_sigma_stats_accumulate): the
per-cell accumulators a run leaves on the device (tasks.sigma_stats_read) turned into time-mean zonal
means and eddy terms per latitude band -- the quantities a Held-Suarez climate is published as."""
import numpy as np

DEFAULT_SIGMA = tuple(round(0.975 - 0.05 * j, 3) for j in range(20))  # 0.975, 0.925, ..., 0.025
MOMENTS = ("u", "v", "T", "uu", "vv", "TT", "uv", "vT")


def band_of(latCell, nbands):
    """the latitude band of each cell: nbands equal bands from the south pole to the north pole"""
    lat = np.asarray(latCell, dtype=np.float64)
    b = np.floor((lat + 0.5 * np.pi) / (np.pi / nbands)).astype(np.int64)
    return np.clip(b, 0, nbands - 1)


def assemble(parts, global_ids, nCells):
    """the accumulators of a decomposed run in global cell order: parts[r] the dict rank r read for its
    owned cells, global_ids[r] their global cell ids (every cell owned by exactly one rank)"""
    out = {}
    for name in parts[0]:
        a = np.zeros((nCells,) + parts[0][name].shape[1:])
        for p, g in zip(parts, global_ids):
            a[np.asarray(g)[:len(p[name])]] = p[name]
        out[name] = a
    return out


def zonal_means(acc, latCell, areaCell, nbands):
    """Zonal and time means per (band, sigma level) from the accumulators `acc` in global cell order
    (a decomposed run: assemble() first, so the result does not depend on the partition).

    Every mean is weighted by cell area times sample count: [X] = sum_c area_c acc_X(c) / sum_c area_c
    n(c) over the band's cells -- fp64 sums over the cells in global cell order.  Returns a dict of
    [nbands, nsigma] arrays: "u", "v", "T" the means; the eddy terms "TT" = [TT] - [T]^2, "uu", "vv",
    "uv" = [uv] - [u][v], "vT" = [vT] - [v][T]; "weight" the denominators; and [nbands] arrays "ps"
    (weighted by area times calls), "lat" (band centres, radians).  A band and level with no sample
    is NaN."""
    lat = np.asarray(latCell, dtype=np.float64).reshape(-1)
    area = np.asarray(areaCell, dtype=np.float64).reshape(-1)
    n = acc["n"]
    nC, ns = n.shape
    if len(lat) != nC or len(area) != nC:
        raise ValueError("zonal_means: latCell, areaCell and the accumulators must cover the same cells")
    band = band_of(lat, nbands)
    cells = [np.nonzero(band == b)[0] for b in range(nbands)]  # (ascending: global cell order)

    def bsum(x):  # per band, the sum over its cells of area * x
        xa = area.reshape((nC,) + (1,) * (x.ndim - 1)) * x
        return np.stack([xa[i].sum(axis=0) if len(i) else np.zeros(x.shape[1:]) for i in cells])

    w = bsum(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = {name: np.where(w > 0.0, bsum(acc[name]) / w, np.nan) for name in MOMENTS}
        wp = bsum(acc["ps"][:, 2])
        ps = np.where(wp > 0.0, bsum(acc["ps"][:, 0]) / wp, np.nan)
    edges = -0.5 * np.pi + (np.pi / nbands) * np.arange(nbands + 1)
    return {"u": m["u"], "v": m["v"], "T": m["T"], "ps": ps,
            "uu": m["uu"] - m["u"] * m["u"], "vv": m["vv"] - m["v"] * m["v"], "TT": m["TT"] - m["T"] * m["T"],
            "uv": m["uv"] - m["u"] * m["v"], "vT": m["vT"] - m["v"] * m["T"],
            "weight": w, "lat": 0.5 * (edges[:-1] + edges[1:])}
