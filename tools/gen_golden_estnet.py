"""TEST INFRASTRUCTURE ONLY -- write tests/golden/estnet.npz by running the reference's EstUnet (archs/Unet.py:474-611) on CPU.

Run where the reference tree exists (not on the GPU box):

    python tools/gen_golden_estnet.py

It imports the reference under the stub modules of `oracle/_refimport.py` (used as is) and stores OUTPUTS and seeds only; the
weights and frames are regenerated from the seeds by tests/estnet_common.py:
  - maps (pge False) of four settings on N = 2 frames of 64 x 96 (tests/estnet_common.MAP_CASES);
  - spatial means of the default network (depth 3, nf 64, 'add', 'std') on the SIDD stack 32 x 256 x 256, its concatenation
    1 x 256 x 8192 and a 1 x 3000 x 4000 frame, with the mean |map| per image and channel (the tolerance's scale);
  - the state_dict keys and shapes of every setting.
  - the reference's own IterDenoise (YOND_SIDD.py:301-483, on `object.__new__(ref.YOND_SIDD)` as oracle/gen_golden.py does) with
    est_type 'pge' + est_net (the SIDD stack with 'iter', a bare 3000 x 4096 frame with 'iter', full_est False from the network)
    and from a PGE.npy table, and 'ours' with est_self.k 19 / est_collab.k 23 (tests/estnet_common.ITER_CASES): every round's
    estimate, crops of every output and its float64 sums.
The reference's forward is run with pge False and the mean is taken as its :610 does (torch.mean over H, W), so one run gives both.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import _refimport  # noqa: E402
import estnet_common as E  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "estnet.npz")
MAP_SEED, MEAN_SEED = 20261016, 7


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same file bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def ref_net(ref, args, sd):
    net = ref.EstUnet(dict(args))
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return net.eval()


def fake_self(ref, pipe, root_dir, est_sections):
    """A reference YOND_SIDD without its constructor (as oracle/gen_golden.py does): the GuidedResUnet nf 8 denoiser, the runfile's
    est_* sections and networks, the dataset root of the table files."""
    import yond_oracle as O
    obj = object.__new__(ref.YOND_SIDD)
    obj.biaslut = None
    obj.device = torch.device('cpu')
    obj.arch = dict(E.GRU8)
    net = getattr(ref, E.GRU8['name'])(dict(E.GRU8))
    obj.net = ref.load_weights(net, O.denoising_state_dict(E.GRU8, E.ITER_DN_SEED), by_name=False).eval()
    obj.pipe = dict(pipe)
    obj.dst = {'root_dir': root_dir}
    obj.args = {k: v[0] for k, v in est_sections.items()}
    obj.est_args = {k: v[0] for k, v in est_sections.items()}
    obj.est_net = {k: v[1] for k, v in est_sections.items()}
    obj.logfile = None
    return obj


def gen_iter_cases(ref, out):
    """(c) pge + est_net / the PGE.npy table, (d) ours: the reference's own IterDenoise (YOND_SIDD.py:301-483) on CPU."""
    import tempfile
    for ci, case in enumerate(E.ITER_CASES):
        name, est_type, hw, full_dn, full_est, it, src, K, s, idx = case
        t0 = time.time()
        pipe = E.iter_pipe(case)
        noisy, beta = E.iter_frame(case)
        tmp = tempfile.mkdtemp()
        sections = {}
        if src == 'net':
            args = dict(E.MEAN_ARGS, weights='')
            net = ref_net(ref, args, E.estimation_weights(E.MEAN_ARGS, E.ITER_EST_SEED, beta))
            sections['est_net'] = (args, net)
        if est_type == 'ours':
            for k, kv in E.OURS_K.items():
                sections[k] = (dict(E.MEAN_ARGS, k=kv, weights=''), object())          # (NeuralNLF never reads the network)
        if src == 'table':
            os.makedirs(os.path.join(tmp, 'SIDD_Validation_Raw'))
            np.save(os.path.join(tmp, 'SIDD_Validation_Raw', 'PGE.npy'), E.pge_table(case))
        obj = fake_self(ref, pipe, tmp, sections)
        p = dict(pipe)
        p.update({'wp': 1023, 'bl': 64, 'ratio': 1, 'gain': 1, 'sigma': 0})
        p['scale'] = (p['wp'] - p['bl']) / p['ratio']
        full_path = None
        if est_type == 'ours':
            full_path = os.path.join(tmp, 'full.npy')
            np.save(full_path, E.iter_full_frame(case))
        data = {'lr_path_full': full_path, 'lr': np.array(np.split(noisy, 32, axis=-1)), 'meta': None, 'name': 'synthetic_000'}
        with torch.no_grad():
            res = obj.IterDenoise(data, {'p': p, 'img_id': 0})
        regs = [np.asarray(r, np.float64) for r in res['regs']]
        out[f"iter_{name}_nout"] = np.int64(len(res['raw_dns']))
        for r_i, r in enumerate(regs):
            out[f"iter_{name}_reg{r_i}"] = r
        for d_i, dn in enumerate(res['raw_dns']):
            dn = np.asarray(dn)
            a, b, c = E.iter_crops(dn)
            out[f"iter_{name}_dn{d_i}_a"], out[f"iter_{name}_dn{d_i}_b"], out[f"iter_{name}_dn{d_i}_c"] = a, b, c
            out[f"iter_{name}_dn{d_i}_sum"] = np.array([dn.astype(np.float64).sum(), (dn.astype(np.float64) ** 2).sum()])
        print(f"iter {name}: {len(res['raw_dns'])} round(s), regs {[r.reshape(-1)[:2].tolist() for r in regs]} in {time.time() - t0:.1f} s",
              flush=True)


def main():
    torch.set_num_threads(8)                  # (a fixed thread count: the same sums in the same order on every run)
    ref = _refimport.import_reference()
    out = {"map_seed": np.int64(MAP_SEED), "mean_seed": np.int64(MEAN_SEED)}
    keys = []
    for ci, (name, args) in enumerate(E.MAP_CASES.items()):
        sd = E.weights(args, MAP_SEED + ci)
        net = ref_net(ref, args, sd)
        keys += [f"{name}:{k}:{'x'.join(map(str, v.shape))}" for k, v in net.state_dict().items()]
        x = torch.from_numpy(E.map_frame(MAP_SEED + ci))[:, None]
        with torch.no_grad():
            y = net(x)
        out[f"map_{name}"] = y.numpy().astype(np.float32)
    args = dict(E.MEAN_ARGS, pge=False)
    sd = E.weights(args, MEAN_SEED)
    net = ref_net(ref, args, sd)
    keys += [f"mean:{k}:{'x'.join(map(str, v.shape))}" for k, v in net.state_dict().items()]
    for name in E.MEAN_CASES:
        t0 = time.time()
        x = torch.from_numpy(E.mean_frame(name, MEAN_SEED))[:, None]
        with torch.no_grad():
            y = net(x)                                     # [N][out_nc][H][W]: the map; :610's mean follows
        out[f"mean_{name}"] = torch.mean(y, dim=(2, 3)).numpy().astype(np.float32)
        out[f"absmean_{name}"] = torch.mean(y.abs().double(), dim=(2, 3)).numpy()
        print(f"{name}: {tuple(x.shape)} in {time.time() - t0:.1f} s", flush=True)
        del y
    gen_iter_cases(ref, out)
    out["keys"] = np.array(keys)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    save_npz(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
