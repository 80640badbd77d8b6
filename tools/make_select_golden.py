"""Records scikit-learn's results on the k-means fixtures of tests/select_cases.py into tests/golden/select_kmeans.npz:

    python tools/make_select_golden.py

Per fixture the labels, the inertia and n_iter of KMeans(n_clusters=k, n_init=10, random_state=0).fit on the float64 matrix, the labels
of the empty-cluster case (init=array, n_init=1), and the scikit-learn version.  No centres are stored.  A fixture is recorded only if
the float64 numpy statement (tests/select_ref64.py) alone reproduces scikit-learn's labels exactly; otherwise the tool stops.  Needs
scikit-learn, which the package itself never imports."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import select_cases as N  # noqa: E402
from tests import select_ref64 as R  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import KMeans
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, make in N.KM_FIXTURES.items():
        x, k = make()
        km = KMeans(n_clusters=k, n_init=10, random_state=0).fit(x)
        ref = R.kmeans(x, k)
        if not np.array_equal(ref["labels"], km.labels_):
            raise SystemExit(f"{name}: the numpy statement's labels differ from scikit-learn's in {int((ref['labels'] != km.labels_).sum())} rows")
        dc = float(np.abs(ref["centers"] + ref["mean"][None, :] - km.cluster_centers_).max())
        print(f"{name}: labels equal; centres differ by {dc:.3g}, inertia by {abs(ref['inertia'] - km.inertia_) / km.inertia_:.3g} relative; "
              f"n_iter {ref['n_iter']} / {km.n_iter_}")
        out[f"{name}_labels"] = km.labels_.astype(np.int16)
        out[f"{name}_inertia"] = np.float64(km.inertia_)
        out[f"{name}_n_iter"] = np.int32(km.n_iter_)
    x, k, init = N.empty_cluster_fixture()
    km = KMeans(n_clusters=k, init=init, n_init=1).fit(x)
    ref = R.kmeans(x, k, init=init)
    if not np.array_equal(ref["labels"], km.labels_):
        raise SystemExit("empty-cluster case: the numpy statement's labels differ from scikit-learn's")
    print(f"empty-cluster case: labels equal, {len(np.unique(km.labels_))} clusters in use")
    out["empty_labels"] = km.labels_.astype(np.int16)
    path = os.path.join(ROOT, "tests", "golden", "select_kmeans.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
