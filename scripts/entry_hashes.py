"""SHA-256 of what the host and sharded entry points of capi.hip and the resident-pair consumers of eigenpair*.hip that
no bit fixture pins return at small fixed inputs, one line per output.
Two builds that issue the same kernels give the same listing on the same GPU: run it on each and diff.
    python scripts/entry_hashes.py [--lib path/to/libflgp_hip.so]"""
import argparse, ctypes, hashlib, os, sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flgp_amd import _lib, api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="hash this build instead of flgp_amd/libflgp_hip.so")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
import torch

L = _lib.lib()
count = 0


def show(name, *arrays):
    global count
    for i, a in enumerate(arrays):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        print(f"{hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}  {name}[{i}] {a.dtype}{list(a.shape)}")
        count += 1


def csr(Z):
    return Z.indices, Z.data


n, d, s, r, K, m, t = 3000, 3, 300, 5, 30, 100, 4.0
X = synth.gaussian_mixture(n, d, seed=808)
U0 = synth.anchors_from_rows(X, synth.random_anchor_rows(n, s, seed=808))
sizes = np.bincount(api.KNN_cpp(X, U0, 1)["ind_knn"][:, 0], minlength=s).astype(float)
U = np.asfortranarray(np.hstack([U0, sizes[:, None]]))
GLS = ("rw", "normalized", "cluster-normalized")
models = dict(kernel="lae", gl="cluster-normalized", root=True)
rng = np.random.default_rng(5)
gathered0, gathered1 = rng.permutation(n)[:700].astype(np.int32), rng.permutation(n)[:90].astype(np.int32)
ranges = np.arange(100, n, dtype=np.int32), np.arange(5, 105, dtype=np.int32)

show("lae", *csr(api.LAE_cpp(X, U0, r)))
for gl in GLS:
    Zl = api.cross_similarity_lae_cpp(X, U, r, gl)
    Zs = api.cross_similarity_se_cpp(X, U, r, gl, 0.7)
    show(f"cross_similarity_lae {gl}", *csr(Zl))
    show(f"cross_similarity_se {gl}", *csr(Zs))
    show(f"graph_laplacian {gl}", *csr(api.graphLaplacian_cpp(api.LAE_cpp(X, U0, r), gl, sizes)))
    for root in (False, True):
        ep = api.spectrum_from_Z_cpp(Zl, K, root)
        show(f"spectrum_from_Z {gl} root={root}", ep.values, ep.vectors)
for kernel, gl, root in (("lae", "cluster-normalized", True), ("se", "rw", False), ("lae", "normalized", False)):
    mo = dict(kernel=kernel, gl=gl, root=root)
    ep = api.heat_kernel_spectrum_cpp(X[:m], X[m:], s, r, K, mo, epsilon=0.7, U=U)
    show(f"heat_kernel_spectrum {kernel} {gl}", ep.values, ep.vectors)
    res = api.heat_kernel_spectrum_resident(X[:m], X[m:], s, r, K, mo, epsilon=0.7, U=U)
    er = res.to_host()
    show(f"heat_kernel_spectrum_resident {kernel} {gl}", er.values, er.vectors)
    show(f"hk_from_eigenpair {kernel} {gl}", res.HK_from_spectrum_cpp(K, t, *ranges), res.HK_from_spectrum_cpp(K, t, gathered0, gathered1))
    res.free()
    for mb in (512, 1):         # one copy; 1 MB blocks of 43 columns (21 per rank of the sharded entry)
        L.flgp_set_tuning(b"hk_block_mb", mb)
        show(f"heat_kernel_covariance {kernel} {gl} hk_block_mb={mb}", api.heat_kernel_covariance_cpp(X[:m], X[m:], s, r, t, K, mo, 1, 0.7, U=U))
        show(f"heat_kernel_covariance_multi [0, 0] {kernel} {gl} hk_block_mb={mb}",
             api.heat_kernel_covariance_cpp(X[:m], X[m:], s, r, t, K, mo, 1, 0.7, U=U, devices=[0, 0]))
    L.flgp_set_tuning(b"hk_block_mb", 512)
ep = api.heat_kernel_spectrum_cpp(X[:m], X[m:], s, r, K, models, U=U)
show("hk_from_spectrum ranges", api.HK_from_spectrum_cpp(ep, K, t, *ranges))
show("hk_from_spectrum gathered", api.HK_from_spectrum_cpp(ep, K, t, gathered0, gathered1))
res = api.ResidentEigenPair.from_host(ep)
show("eigenpair_from_host -> hk_from_eigenpair", res.HK_from_spectrum_cpp(K, t, *ranges))
# the resident-pair consumers that no bit fixture pins (csrc/eigenpair*.hip): m <= K and m > K, rows in place and gathered
Yr, Yt, Yb = rng.standard_normal((100, 2)), rng.standard_normal(n), (rng.random(100) < 0.5).astype(float)
for rows, tr, new in (("ranges", ranges[1], ranges[0]), ("gathered", gathered0, gathered1)):
    for mm in (20, 100):
        i0, y, yb, tag = tr[:mm], Yr[:mm], Yb[:mm], f"{rows} m={mm}"
        noises = 0.1 + 0.05 * np.arange(mm) / mm
        show(f"VtV VtY VC {tag}", res.VtV(K, i0), res.VtY(K, i0, y), res.VC(K, i0, Yr[:K]))
        show(f"predict_regression same different {tag}", res.predict_regression_cpp(y, i0, new, K, (t, 0.1), 1e-3),
             res.predict_regression_cpp(y, i0, new, K, (t, *noises), 1e-3, "different"))
        show(f"posterior_covariance_regression {tag}", res.posterior_covariance_regression(i0, new, K, (t, 0.1), 1e-3))
        rp = res.regression_posterior(y[:, 0], i0, new, K, (t, 0.1), 1e-3, target=Yt[:new.size])
        show(f"regression_posterior {tag}", rp["Y_pred"]["train"], rp["Y_pred"]["test"], rp["posterior"]["cov"], np.array([rp["nll"]]))
        show(f"marginal_log_likelihood_logit_la {tag}", np.array(res.marginal_log_likelihood_logit_la(K, t, i0, yb, return_iters=True)))
        pc = res.posterior_distribution_classification(i0, new, K, t, yb, 1e-3, 1e-3)
        show(f"posterior_distribution_classification {tag}", pc["mean"], pc["cov"])
res.free()
em = api.lae_eigenmap(X, s, r, 4, U=U)
show("lae_eigenmap", em["eigenvalues"], em["eigenvectors"])
ny = api.nystrom_eigenpair_cpp(X, U0, 1.0, K)
show("nystrom_eigenpair", ny.values, ny.vectors)
res = api.nystrom_eigenpair_cpp(X, U0, 1.0, K, resident=True)
er = res.to_host()
show("nystrom_eigenpair_resident", er.values, er.vectors)
res.free()

# the device entries, on device copies of the same points / anchors / sizes (column-major: a (k, n) tensor)
dev = "cuda:0"
cm = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(dev)     # noqa: E731
dX, dU, dsz = cm(X), cm(U0), torch.from_numpy(sizes).to(dev)
st = torch.cuda.current_stream().cuda_stream
a2s = np.array([0.1, 1.0, 10.0])
for gl in GLS:
    for root in (False, True):
        pairs, mean = api.se_spectrum_grid(X[:m], X[m:], s, r, K=K, a2s=a2s, models=dict(gl=gl, root=root), U=U, max_parallel=3)
        show(f"se_spectrum_grid {gl} root={root}", np.array([mean]), *[p.values for p in pairs], *[p.vectors for p in pairs])
        vals = torch.zeros((3, K), dtype=torch.float64, device=dev); vecs = torch.zeros((3, K, n), dtype=torch.float64, device=dev)
        iters = (ctypes.c_int * 3)(); dmean = ctypes.c_double(0.0)
        _lib.check(L.flgp_dev_se_spectrum_grid(st, dX.data_ptr(), n, n, d, dU.data_ptr(), s, s, dsz.data_ptr(), r, K, a2s.ctypes.data, 3,
                                               gl.encode(), int(root), vals.data_ptr(), vecs.data_ptr(), ctypes.addressof(dmean), 3,
                                               ctypes.addressof(iters)))
        show(f"dev_se_spectrum_grid {gl} root={root}", np.array([dmean.value]), np.array(list(iters)), vals, vecs)
dcs = torch.zeros(s, dtype=torch.float64, device=dev)
_lib.check(L.flgp_dev_cluster_sizes(st, None, dX.data_ptr(), n, n, d, dU.data_ptr(), s, s, dcs.data_ptr()))
show("dev_cluster_sizes", dcs)
for kernel, gl, root in (("lae", "cluster-normalized", True), ("se", "rw", False)):
    dH = torch.zeros((m, n), dtype=torch.float64, device=dev); dval = torch.zeros(K, dtype=torch.float64, device=dev)
    dvec = torch.zeros((K, n), dtype=torch.float64, device=dev); info = (ctypes.c_int * 4)()
    _lib.check(L.flgp_dev_heat_kernel_covariance_sharded(st, None, dX.data_ptr(), n, n, d, n, 0, dU.data_ptr(), s, s, dcs.data_ptr(), m, r, t, K,
                                                         kernel.encode(), gl.encode(), int(root), 0.7, dH.data_ptr(), n, dval.data_ptr(),
                                                         dvec.data_ptr(), n, ctypes.addressof(info)))
    show(f"dev_heat_kernel_covariance_sharded world 1 {kernel} {gl}", dH, dval, dvec, np.array(list(info)))
print(f"{count} hashes")
