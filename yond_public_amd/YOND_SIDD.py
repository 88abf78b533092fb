"""Evaluation entry point with the reference's surface (YOND_SIDD.py:136-236, 485-570, 723-744):

    python YOND_SIDD.py -f runfiles/YOND/SIDD_simple+full_pre_grumix.yml -m eval
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 YOND_SIDD.py -f ... -m eval

Same runfile schema (`pipeline`, `dst*`, `arch`), same class / method names (`YOND_SIDD.eval`, `IterDenoise`,
`VST_Denoiser`, `Simple_Denoiser`), same model lookup by name and checkpoint search order.  Differences that
are the point of this build: every per-pixel pass runs on the MI355X HIP kernels; images are sharded one per
GPU process (image k -> rank k mod world) instead of nn.DataParallel over batch 1; per-block PSNR/SSIM are
computed on the device and reduced with ONE all-reduce at the end.  `--fig` turns the reference's save_plot on (`--nofig` is
`store_true` with default True there too, so it can never be turned off: :731): frames rendered to sRGB by the HIP kernel
(yond_public_amd/isp.py), PNGs under the sample directory, PSNR(sRGB) / SSIM(sRGB) beside the raw metrics (:635-677, 551-563).

Datasets: the reference's SIDD layout (`<root_dir>/SIDD_Validation_Raw/Validation{Noisy,Gt}BlocksRaw.mat`, MATLAB v5, plus
`SIDD_Benchmark_Data/*/*_010.MAT` metadata: yond_public_amd/data.py mirrors data_process/yond_datasets.py:767-868), or
`<root_dir>/npy/{noisy,gt}_{k:03d}.npy` ((32,256,256) float32 in [0,1], plus optional `full_{k:03d}.npy`); DNG / ARW and
MATLAB v7.3 need rawpy / h5py, which this image lacks.  Without data the driver evaluates seeded synthetic stand-ins so
the whole control flow can be exercised and timed.
"""
import argparse
import os
import time
from pathlib import Path

import numpy as np
import torch
import yaml

from . import archs as _archs
from . import distributed as D
from . import pipeline as P
from . import synthetic as S


def log(string, log=None, notime=False):
    s = f'{time.strftime("%Y-%m-%d %H:%M:%S")} >>  {string}' if not notime else string
    print(s, flush=True)
    if log is not None:
        with open(log, 'a+') as f:
            f.write(s + '\n')


class SyntheticSIDD:
    """Stand-in for SIDD_Dataset (data_process/yond_datasets.py:767-868): items with 'lr', 'hr' of shape
    (32, 256, 256), 'lr_full' (the frame used for the round-1 estimate: 3000 x 5328, the size SURVEY 8d names for the
    stand-ins of the SIDD full frames), 'name'."""

    def __init__(self, n=40, K=4.0, sigma=6.0, full_hw=(3000, 5328), distinct=8):
        """distinct: item k is the synthesis of seed k % distinct, kept once made (a 16 MP Poisson draw takes ~1 s of NumPy -- 300 x the
        GPU time of the image; a real dataset's items come from files, which the loader threads overlap with the GPU)."""
        self.n, self.K, self.sigma, self.full_hw, self.distinct = n, K, sigma, full_hw, max(1, distinct)
        self._made = {}

    def prepare(self, indices=None, workers=8):
        """Synthesise the distinct items up front, in parallel -- the counterpart of SIDD_Dataset.__init__ reading the validation blocks
        before the evaluation loop starts (data_process/yond_datasets.py:797-806); afterwards an item costs no host arithmetic."""
        from concurrent.futures import ThreadPoolExecutor
        need = sorted({k % self.distinct for k in (indices if indices is not None else range(self.n))} - set(self._made))
        if need:
            with ThreadPoolExecutor(max_workers=min(workers, len(need))) as ex:
                list(ex.map(self.__getitem__, need))

    def __len__(self):
        return self.n

    def item_size(self, k):
        return self.full_hw[0] * self.full_hw[1]

    def __getitem__(self, k):
        j = k % self.distinct
        if j not in self._made:
            noisy, clean = S.synth_noisy(256, 8192, self.K, self.sigma, 100 + j)
            full, _ = S.synth_noisy(self.full_hw[0], self.full_hw[1], self.K, self.sigma, 500 + j)
            self._made[j] = (np.array(np.split(noisy, 32, axis=-1)), np.array(np.split(clean, 32, axis=-1)), full)
        lr, hr, full = self._made[j]
        return {'lr': lr, 'hr': hr, 'lr_full': full, 'name': f'synthetic_{k:03d}', 'meta': None, 'cfa': 'rggb'}


class NpySIDD:
    def __init__(self, root):
        self.root = root
        self.ids = sorted(int(p.stem.split('_')[1]) for p in Path(root).glob('noisy_*.npy'))

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        k = self.ids[i]
        d = {'lr': np.load(f'{self.root}/noisy_{k:03d}.npy').astype(np.float32), 'name': f'sidd_{k:03d}', 'meta': None, 'cfa': 'rggb'}
        if os.path.exists(f'{self.root}/gt_{k:03d}.npy'):
            d['hr'] = np.load(f'{self.root}/gt_{k:03d}.npy').astype(np.float32)
        d['lr_full'] = np.load(f'{self.root}/full_{k:03d}.npy').astype(np.float32) if os.path.exists(f'{self.root}/full_{k:03d}.npy') else None
        return d


def load_estimators(args, device, logfile=None, beta=(4.0 / 959, 6.0 / 959)):
    """YOND_SIDD.py:187-196: every top-level runfile key that contains 'est_' is one network, built by name from
    yond_public_amd.archs with the section as its arguments and loaded from section['weights'].  A missing weights file is
    logged and replaced by deterministic estimation weights (synthetic.estimation_state_dict: conv_final's bias = beta, the
    (beta1, sqrt(beta2)) of the synthetic stand-in frames), as the denoiser's missing checkpoint is.  Returns (sections, networks)."""
    est_args = {key: args[key] for key in args if 'est_' in key}
    est_net = {}
    for name, sec in est_args.items():
        cls = getattr(_archs, str(sec.get('name')), None)
        if cls is None:
            raise SystemExit(f"runfile section {name}: no network {sec.get('name')!r} in yond_public_amd.archs")
        net = cls(sec)
        path = sec.get('weights')
        if path and os.path.exists(path):
            # load_weights(by_name=False) (utils/utils.py:160-204): the checkpoint's entries over the model's own state_dict, so a
            # checkpoint without some of the model's keys (noiseSTD, say) loads; a key the model does not have still raises
            state = net.state_dict()
            state.update(torch.load(path, map_location='cpu'))
            net.load_state_dict(state)
            src = path
        else:
            net.load_state_dict(S.estimation_state_dict(net, beta))
            src = f"{path} not found -> synthetic estimation weights"
        est_net[name] = net.to(device).eval()
        log(f'Estimator {name}:\t{sec.get("name")} ({src})', logfile, notime=True)
    return est_args, est_net


class YOND_SIDD:
    on_result = None               # callable(name, res): called with every image's result right before it is accounted

    def __init__(self, args=None):
        self.parser = YONDParser().parse(args)
        if getattr(self.parser, 'synth_noise', None) is not None:
            raise SystemExit("--synth-noise belongs to the full-frame drivers (YOND_any / YOND_ELD / YOND_LRID / YOND_DND): YOND_SIDD's block layout "
                             "(32 blocks per image, the estimate on the full frame) is a different loop and has no synthetic-noise path")
        if getattr(self.parser, 'camera_noise', None) is not None:
            raise SystemExit("--camera-noise belongs to the full-frame drivers (YOND_any / YOND_ELD / YOND_LRID / YOND_DND): YOND_SIDD's block layout "
                             "(32 blocks per image, the estimate on the full frame) is a different loop and has no synthetic-noise path")
        if getattr(self.parser, 'illum_corr', None) not in (None, 'off'):
            raise SystemExit("--illum-corr belongs to the full-frame drivers (YOND_any / YOND_ELD / YOND_LRID): the ELD protocol's brightness alignment is "
                             "a whole-frame step, YOND_SIDD's metrics are per block")
        if getattr(self.parser, 'noise_kld', None) is not None:
            raise SystemExit("--noise-kld belongs to the full-frame drivers (YOND_any / YOND_ELD / YOND_LRID): the residual histogram is taken over a whole "
                             "paired frame, YOND_SIDD's loop works on blocks")
        if getattr(self.parser, 'bad_pixels', None) is not None or getattr(self.parser, 'synth_defects', None) is not None:
            raise SystemExit("--bad-pixels / --synth-defects belong to the full-frame drivers (YOND_any / YOND_ELD / YOND_LRID): the repair works on a "
                             "whole Bayer mosaic, YOND_SIDD's (and YOND_DND's) loop is handed packed blocks")
        if getattr(self.parser, 'row_denoise', None) is not None:
            raise SystemExit("--row-denoise belongs to the full-frame drivers (YOND_any / YOND_ELD / YOND_LRID): the row means are taken over a whole "
                             "Bayer mosaic, YOND_SIDD's (and YOND_DND's) loop is handed packed blocks")
        self.initialization()

    def initialization(self):
        with open(self.parser.runfile, 'r', encoding='utf-8') as f:
            self.args = yaml.load(f.read(), Loader=yaml.FullLoader)
        self.mode = self.args['mode'] if self.parser.mode is None else self.parser.mode
        self.rank, self.local_rank, self.world = D.init()
        if not torch.cuda.is_available():
            raise SystemExit("YOND_SIDD needs an MI355X: the HIP path has no CPU fallback")
        self.device = torch.device('cuda', self.local_rank)
        torch.cuda.set_device(self.device)
        self.dst, self.arch, self.pipe = self.args['dst'], self.args['arch'], self.args['pipeline']
        if self.pipe['bias_corr'] == 'none':
            self.pipe['bias_corr'] = None
        if getattr(self.parser, 'fit', None) is not None:                            # --fit overrides the runfile's pipeline.est_fit
            self.pipe['est_fit'] = self.parser.fit
        P.est_fit_of(self.pipe)                                                      # ('ransac': no device chain, images one at a time)
        self.model_name, self.method_name = self.args['model_name'], self.args['method_name']
        self.fast_ckpt = self.args['fast_ckpt']
        self.save_plot = bool(getattr(self.parser, 'fig', False))                    # YOND_SIDD.py:153
        self.sample_dir = os.path.join(str(self.args.get('result_dir', './images')), f"{self.method_name}")        # :170
        os.makedirs('./logs', exist_ok=True)
        self.logfile = f'./logs/log_{self.method_name}.log' if self.rank == 0 else None
        # model: looked up by name, checkpoint search order best -> last -> plain (YOND_SIDD.py:177-184)
        self.net = getattr(_archs, self.arch['name'])(self.arch)
        for suffix in ('_best_model.pth', '_last_model.pth', '.pth'):
            model_path = f'{self.fast_ckpt}/{self.model_name}{suffix}'
            if os.path.exists(model_path):
                state = torch.load(model_path, map_location='cpu')
                self.net.load_state_dict(state)
                break
        else:
            model_path = None                      # no checkpoint: a deterministic weak denoiser (both rounds run)
            self.net.load_state_dict(S.denoising_state_dict(self.net, 0))
        self.net = self.net.to(self.device).eval()
        self.est_args, self.est_net = load_estimators(self.args, self.device, self.logfile if self.rank == 0 else None)
        # the 2-D bias LUT when its blob is present (YOND_SIDD.py:171), else get_bias per image
        self.biaslut = P.BiasLUT() if os.path.exists('checkpoints/bias_lut_2d.npy') else None
        if self.rank == 0:
            nparam = sum(p.numel() for p in self.net.parameters())
            log(f'Method Name:\t{self.method_name}', self.logfile, notime=True)
            log(f'Architecture:\t{self.arch["name"]}', self.logfile, notime=True)
            log(f'Parameters:\t{nparam / 1e6:.2f}M', self.logfile, notime=True)
            log(f'Checkpoint:\t{model_path or "none found -> synthetic denoising weights (timing / parity only)"}', self.logfile, notime=True)
            log(f"Let's use {self.world} GPUs (one process each, image-parallel)!", self.logfile, notime=True)
        self.change_eval_dst('eval')

    def change_eval_dst(self, mode='eval'):
        self.dst = self.args[f'dst_{mode}']
        root = os.path.join(self.dst['root_dir'], 'npy')
        mat = os.path.join(self.dst['root_dir'], 'SIDD_Validation_Raw',
                           'ValidationNoisyBlocksRaw.mat' if mode == 'eval' else 'BenchmarkNoisyBlocksRaw.mat')
        if os.path.exists(mat):                       # the reference's layout (data_process/yond_datasets.py:797-806)
            from .data import SIDD_Dataset
            self.dst_eval = SIDD_Dataset(dict(self.dst, mode=mode))
        elif os.path.isdir(root) and list(Path(root).glob('noisy_*.npy')):
            self.dst_eval = NpySIDD(root)
        else:
            self.dst_eval = SyntheticSIDD(self.parser.synthetic)

    # -- reference method names -----------------------------------------------------------------
    def Simple_Denoiser(self, lr_raw):
        return P.Simple_Denoiser(lr_raw, self.net, device=self.device)

    def VST_Denoiser(self, lr_raw, hr_raw=None, bias_corr='pre', bias_func=None, denoiser='gru32n', p=None):
        return P.VST_Denoiser(lr_raw, p, self.net, self.arch, bias_corr, bias_func, self.pipe.get('vst_type', 'exact'),
                              device=self.device, biaslut=self.biaslut, denoiser=denoiser if denoiser in ('fbi', 'bm3d') else None)

    def _est(self, data, params):
        """What IterDenoise's estimate may read: the dataset tree and image (file estimates), the est_* sections and their networks."""
        return {'root_dir': (getattr(self, 'dst', None) or {}).get('root_dir'), 'img_id': params.get('img_id'), 'name': data.get('name'),
                'est_net': (getattr(self, 'est_net', None) or {}).get('est_net'), 'est_args': getattr(self, 'est_args', None) or {}}

    def IterDenoise(self, data, params):
        # data['lr'] is the [32][256][256] stack; pipeline.IterDenoise concatenates it for the estimate (:315) and, with
        # pipe['full_dn'], for the denoiser (:388); the collaborative estimate re-tiles per block (SIDD_256, :431)
        res = P.IterDenoise(data['lr'], self.net, self.arch, self.pipe, lr_full=data.get('lr_full'), p=params['p'],
                            device=self.device, log=(lambda s: log(s, self.logfile)) if self.parser.verbose else None,
                            biaslut=self.biaslut,
                            est=self._est(data, params))
        cat = lambda a: torch.cat(list(a), dim=-1) if isinstance(a, torch.Tensor) else np.concatenate(a, axis=-1)   # (:480-481)
        res['lr_raw'] = cat(data['lr'])
        res['hr_raw'] = cat(data['hr']) if data.get('hr') is not None else None
        return res

    def IterDenoiseGroup(self, datas, params_list):
        """IterDenoise for several items at once (pipeline.IterDenoiseGroup): round 1 of the G images as ONE batch-(32 G) forward, round 2
        likewise; every image keeps its own estimates, tables and t, and its result is IterDenoise's.  The reference takes the
        images one by one (:507-514); they are independent, and 32 blocks of 128 x 128 packed pixels leave the deep levels of a forward
        (16 x 16 and 8 x 8 pixels) far too small for the chip."""
        ress = P.IterDenoiseGroup([(d['lr'], d.get('lr_full')) for d in datas], self.net, self.arch, self.pipe, ps=[q['p'] for q in params_list],
                                  device=self.device, log=(lambda s: log(s, self.logfile)) if self.parser.verbose else None, biaslut=self.biaslut,
                                  ests=[self._est(d, q) for d, q in zip(datas, params_list)])
        cat = lambda a: torch.cat(list(a), dim=-1) if isinstance(a, torch.Tensor) else np.concatenate(a, axis=-1)   # (:480-481)
        for res, d in zip(ress, datas):
            res['lr_raw'] = cat(d['lr'])
            res['hr_raw'] = cat(d['hr']) if d.get('hr') is not None else None
        return ress

    # -- sRGB rendering (--fig) -----------------------------------------------------------------
    @staticmethod
    def _fig_tag(name):
        """name[:4] (YOND_SIDD.py:638: the SIDD scene number); the whole name where that is no number (the stand-ins)."""
        return name[:4] if name[:4].isdigit() else name

    def _render(self, data, raw):
        """process_sidd_image of one Bayer frame with the item's metadata -> device uint8 [H][W][3] RGB.  Items without metadata (the
        synthetic stand-ins, .npy blocks) render as RGGB with wb = 1 and the identity as the camera -> sRGB matrix."""
        from . import isp
        if data.get('meta') is not None and data.get('wb') is not None and data.get('ccm') is not None:
            return isp.render_sidd(raw, data['cfa'], data['wb'], data['ccm'], order='rgb')
        return isp.render_sidd(raw, isp.RGGB, [[1.0, 1.0, 1.0]], None, order='rgb', ccm=np.eye(3))

    def _save_png(self, path, img):
        """PNG encoding on a host thread: the device goes on with the next image."""
        from concurrent.futures import ThreadPoolExecutor
        from . import isp
        if getattr(self, '_png_pool', None) is None:
            self._png_pool, self._png_jobs = ThreadPoolExecutor(max_workers=2), []
        os.makedirs(os.path.dirname(path), exist_ok=True)
        self._png_jobs.append(self._png_pool.submit(isp.save_png, path, img.cpu().numpy()))

    def _png_wait(self):
        for job in getattr(self, '_png_jobs', None) or []:
            job.result()
        self._png_jobs = []

    def figures(self, data, res):
        """multiprocess_plot's save_plot part (YOND_SIDD.py:635-677) for one image: the concatenated 256 x 8192 noisy frame, the ground
        truth and every round's output rendered whole (the demosaic crosses the block seams as in the reference), written as PNGs, and
        the per-image sRGB metrics over the 32 blocks along the width.  Returns (psnrs_rgb, ssims_rgb), None where a round was skipped."""
        from . import isp
        tag = self._fig_tag(data['name'])
        self._save_png(f'{self.sample_dir}/{tag}_noisy.png', self._render(data, res['lr_raw']))
        img_hr = None
        if res.get('hr_raw') is not None:
            img_hr = self._render(data, res['hr_raw'])
            self._save_png(f'{self.sample_dir}/{tag}_gt.png', img_hr)
        psnrs, ssims = [], []
        for it, dn in enumerate(res['raw_dns']):
            if float(dn.max()) <= 0:                                                   # :644-647
                psnrs.append(None)
                ssims.append(None)
                continue
            img_dn = self._render(data, dn)
            self._save_png(f'{self.sample_dir}/{tag}_{it}.png', img_dn)
            if img_hr is not None:
                ps, ss = isp.block_metrics_rgb(img_dn, img_hr, 256, img_dn.shape[1] // 32)          # :661-665
                psnrs.append(float(np.mean(ps)))
                ssims.append(float(np.mean(ss)))
        return psnrs, ssims

    def _groups(self, it):
        """The prefetcher's items `group` at a time (consecutive items; the last group may be short)."""
        G = max(1, int(getattr(self.parser, 'group', 1)))
        batch = []
        for k, data in it:
            batch.append((k, data))
            if len(batch) == G:
                yield batch
                batch = []
        if batch:
            yield batch

    def eval(self, epoch=-1):
        """`--save f32` keeps every image's rounds as the reference does (YOND_SIDD.py:512-536): npy/<method_name>/<k:03d>.npy, float32
        [max_iter + 1][256][8192] (rounds that did not run stay zero), written behind the GPU loop by a rawio.FrameWriter."""
        save = getattr(self.parser, 'save', 'none')
        if save == 'dn16':
            raise SystemExit("YOND_SIDD eval keeps the reference's float32 cache: use --save f32")
        writer = None
        if save == 'f32':
            from .rawio import FrameWriter
            writer = FrameWriter(f'npy/{self.method_name}', 'f32')
        try:
            return self._eval(writer)
        finally:
            if writer is not None:
                writer.close()

    def _eval(self, writer):
        n_it = self.pipe['max_iter'] + 1 if self.pipe.get('iter') == 'iter' else 1
        fig = bool(getattr(self, 'save_plot', False))        # --fig: everything below is today's path without it
        sums = D.MetricSums(n_it, rgb=True) if fig else D.MetricSums(n_it)
        p = dict(self.pipe)
        p.update({'wp': 1023, 'bl': 64, 'ratio': 1, 'gain': 1, 'sigma': 0})          # YOND_SIDD.py:504
        p['scale'] = (p['wp'] - p['bl']) / p['ratio']
        mine = D.shard_dataset(self.dst_eval, self.rank, self.world)        # size-aware (five phones, five frame sizes) where sizes are known
        self.metrics = {}
        if hasattr(self.dst_eval, 'prepare'):
            self.dst_eval.prepare(mine)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_path = 0.0
        marks = []                                          # (wall clock, path seconds so far) behind every image: the steady state is the second half
        # the items are read and uploaded by loader threads ahead of the GPU (the reference reads each in front of its IterDenoise,
        # :507-514): file reads, the float32 conversion and the 64 MB upload of the full frame overlap the previous images' kernels
        from .data import Prefetcher
        G = max(1, int(getattr(self.parser, 'group', 1)))
        pf = Prefetcher(self.dst_eval, mine, self.device, depth=max(self.parser.prefetch, 3 * G), workers=self.parser.loaders)
        est_type = str(self.pipe.get('est_type', 'simple'))
        streamed = (P.STREAM_GROUPS and getattr(self.parser, 'stream', True) and self.pipe.get('iter') == 'iter' and self.pipe.get('max_iter', 1) == 1
                    and 'simple' in est_type and 'cal_est' not in self.pipe and 'rot_cfa' not in p and self.biaslut is None)
        if fig:
            streamed = False                                 # the figures are rendered image by image behind IterDenoise

        def metrics_of(data, res):
            psnrs, ssims = [], []
            hr_raw = data.get('hr')
            if hr_raw is not None:
                hr = torch.cat(list(hr_raw), dim=-1) if isinstance(hr_raw, torch.Tensor) else torch.from_numpy(np.concatenate(hr_raw, axis=-1)).to(self.device)
                for dn in res['raw_dns']:
                    ps, ss = P.block_metrics(dn, hr)                                   # :649-652 per 256x256 block
                    psnrs.append(float(np.mean(ps)))
                    ssims.append(float(np.mean(ss)))
            return psnrs, ssims

        def keep(k, data, res):
            if callable(self.on_result):
                self.on_result(data['name'], res)
            if writer is not None:
                dns = res['raw_dns']
                outputs = torch.zeros((n_it,) + tuple(dns[0].shape), dtype=torch.float32, device=dns[0].device)      # :512
                for it, dn in enumerate(dns):
                    outputs[it].copy_(dn)
                writer.put(f'{k:03d}', outputs, (p['bl'], p['wp'], p['ratio']),
                           {'name': data['name'], 'rounds': [(float(q[0]), float(q[1])) for q in res.get('params', [])]})

        def account(data, res, psnrs, ssims):
            if not fig:
                if psnrs:
                    sums.update(psnrs, ssims)            # iterations that did not run count -1 in their own meter (:644-647)
                self.metrics[data['name']] = {'psnr': psnrs, 'ssim': ssims, 'reg': res['regs']}
            else:
                if 'lr_raw' not in res:
                    cat = lambda a: torch.cat(list(a), dim=-1) if isinstance(a, torch.Tensor) else np.concatenate(a, axis=-1)
                    res['lr_raw'], res['hr_raw'] = cat(data['lr']), cat(data['hr']) if data.get('hr') is not None else None
                psnrs_rgb, ssims_rgb = self.figures(data, res)
                done = [(a, b) for a, b in zip(psnrs_rgb, ssims_rgb) if a is not None]
                if psnrs and done:
                    sums.update(psnrs, ssims, psnrs_rgb, ssims_rgb)
                self.metrics[data['name']] = {'psnr': psnrs, 'ssim': ssims, 'reg': res['regs'],
                                              'psnr_rgb': [a for a, _ in done], 'ssim_rgb': [b for _, b in done]}
            log(f"[rank {self.rank}] {data['name']}: PSNR={psnrs[-1] if psnrs else float('nan'):.2f}, "
                f"SSIM={ssims[-1] if ssims else float('nan'):.4f}", self.logfile)
            if fig and done:
                log(f"PSNR(sRGB)={done[-1][0]:.2f}, SSIM(sRGB)={done[-1][1]:.4f}", self.logfile)           # :677

        if streamed:
            # consecutive groups overlapped on two HIP streams (pipeline.denoise_stream_groups): group k+1's full-frame estimates under group k's first
            # pass, group k's collaborative estimates under group k-1's second; the block metrics of a finished group on a third stream
            batches, done = {}, {}

            def groups():
                for gi, batch in enumerate(self._groups(pf)):
                    batches[gi] = batch
                    yield [(d['lr'], d.get('lr_full')) for _, d in batch]

            def finish(gi, ress):
                done[gi] = [metrics_of(d, r) for (_, d), r in zip(batches[gi], ress)]

            for gi, ress in enumerate(P.denoise_stream_groups(groups(), self.net, self.arch, self.pipe, p=dict(p, cfa=[[1, 2], [2, 3]]), device=self.device,
                                                             log=(lambda s: log(s, self.logfile)) if self.parser.verbose else None, finish=finish)):
                batch = batches.pop(gi)
                for (k, data), res, (psnrs, ssims) in zip(batch, ress, done.pop(gi)):
                    keep(k, data, res)
                    account(data, res, psnrs, ssims)
                t_path = time.perf_counter() - t0          # (groups overlap: the path IS the wall clock here)
                marks.extend([(time.perf_counter(), t_path)] * len(batch))
        else:
          for batch in self._groups(pf):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            datas = [d for _, d in batch]
            plist = [{'p': dict(p, cfa=d.get('cfa', [[1, 2], [2, 3]])), 'img_id': k} for k, d in batch]      # YOND_SIDD.py:510
            if len(batch) == 1:
                ress = [self.IterDenoise(datas[0], plist[0])]
            else:
                ress = self.IterDenoiseGroup(datas, plist)
            for (k, data), res in zip(batch, ress):
                psnrs, ssims = metrics_of(data, res)
                keep(k, data, res)
                account(data, res, psnrs, ssims)
            torch.cuda.synchronize()
            t_path += time.perf_counter() - t1              # estimate + denoise (+ metrics) of this group's images
            marks.extend([(time.perf_counter(), t_path)] * len(batch))
        torch.cuda.synchronize()
        self._png_wait()
        dt = time.perf_counter() - t0
        red = sums.reduce(self.device)                 # the ONE collective of the eval path (RCCL over xGMI)
        dt = D.max_over_ranks(dt, self.device)
        if self.rank == 0:
            log(f'{self.method_name}:', self.logfile)
            for it in range(n_it):
                log(f"Iter{it}: PSNR={red[f'psnr_iter{it}']:.2f}, SSIM={red[f'ssim_iter{it}']:.4f}", self.logfile)
                if fig:                                                       # :555-557
                    log(f"PSNR(sRGB)={red[f'psnr_rgb_iter{it}']:.2f}, SSIM(sRGB)={red[f'ssim_rgb_iter{it}']:.4f}", self.logfile, notime=True)
            log(f"Iter_last: PSNR={red['psnr_last']:.2f}, SSIM={red['ssim_last']:.4f}", self.logfile)
            if fig:                                                           # :561-563
                log(f"PSNR(sRGB)={red['psnr_rgb_last']:.2f}, SSIM(sRGB)={red['ssim_rgb_last']:.4f}", self.logfile, notime=True)
            log(f"{red['count']} images on {self.world} GPU(s) in {dt:.2f} s "
                f"(rank 0: {dt / max(len(mine), 1) * 1e3:.1f} ms wall per image, {t_path / max(len(mine), 1) * 1e3:.1f} ms of it in IterDenoise + metrics; "
                f"the rest is waiting for the {self.parser.loaders} loader threads)", self.logfile)
            self.last_timing = {'wall_ms_per_image': dt / max(len(mine), 1) * 1e3, 'path_ms_per_image': t_path / max(len(mine), 1) * 1e3}
            if len(marks) >= 8:
                h = len(marks) // 2                           # second half: lazily built plans / buffers and the loaders' start-up are behind us
                wall2 = (marks[-1][0] - marks[h - 1][0]) / (len(marks) - h) * 1e3
                path2 = (marks[-1][1] - marks[h - 1][1]) / (len(marks) - h) * 1e3
                self.last_timing.update(steady_wall_ms_per_image=wall2, steady_path_ms_per_image=path2)
                log(f"steady state (second half of rank 0's images): {wall2:.2f} ms wall per image, {path2:.2f} ms of it in IterDenoise + metrics "
                    f"(x{wall2 / max(path2, 1e-9):.2f})", self.logfile)
            log(f"collectives: backend={D.STATS['backend']}, all_reduce={D.STATS['all_reduce']}, barrier={D.STATS['barrier']}", self.logfile)
        return red


    def benchmark(self):
        """YOND_SIDD.py:572-630 (`-m test`): the SIDD BENCHMARK blocks (no ground truth) through IterDenoise; keeps what the
        reference keeps -- per-image estimates as `reg_test` in self.metrics and the two submission arrays
        bench_init / bench_results [N][32][256][256] (first / last round) -- and writes them to npy/<method>/ (the reference's
        .mat export is commented out upstream, :615-621).  With --fig the noisy frame and every round's output are rendered to
        sRGB and written as <sample_dir>/benchmark/<name[:4]>_noisy.png and _<it>.png (:600-608).  Images are sharded over the ranks;
        every rank writes the blocks of its own images."""
        n = len(self.dst_eval)
        bench_init = np.zeros((n, 32, 256, 256), np.float32)
        bench_results = np.zeros((n, 32, 256, 256), np.float32)
        p = dict(self.pipe)
        p.update({'wp': 1023, 'bl': 64, 'ratio': 1, 'gain': 1, 'sigma': 0})                  # :586
        p['scale'] = (p['wp'] - p['bl']) / p['ratio']
        self.metrics = getattr(self, 'metrics', None) or {}
        mine = D.shard_dataset(self.dst_eval, self.rank, self.world)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        from .data import Prefetcher
        G = max(1, int(getattr(self.parser, 'group', 1)))
        for batch in self._groups(Prefetcher(self.dst_eval, mine, self.device, depth=max(self.parser.prefetch, 2 * G), workers=self.parser.loaders)):
            datas = [d for _, d in batch]
            plist = [{'p': dict(p, cfa=d.get('cfa', [[1, 2], [2, 3]])), 'img_id': k} for k, d in batch]
            ress = [self.IterDenoise(datas[0], plist[0])] if len(batch) == 1 else self.IterDenoiseGroup(datas, plist)
            for (k, data), res in zip(batch, ress):
                self.metrics.setdefault(data['name'], {})['reg_test'] = res['regs']                   # :597
                first, last = res['raw_dns'][0].cpu().numpy(), res['raw_dns'][-1].cpu().numpy()
                bench_init[k] = np.array(np.split(first, 32, axis=-1))                                # :612-613
                bench_results[k] = np.array(np.split(last, 32, axis=-1))
                if getattr(self, 'save_plot', False):                                                 # :600-608
                    tag = self._fig_tag(data['name'])
                    self._save_png(f'{self.sample_dir}/benchmark/{tag}_noisy.png', self._render(data, res['lr_raw']))
                    for it, dn in enumerate(res['raw_dns']):
                        if float(dn.max()) > 0:
                            self._save_png(f'{self.sample_dir}/benchmark/{tag}_{it}.png', self._render(data, dn))
                log(f"[rank {self.rank}] {data['name']}: {len(res['raw_dns'])} round(s), regs {[tuple(float(v) for v in r) for r in res['regs']]}", self.logfile)
        torch.cuda.synchronize()
        self._png_wait()
        dt = D.max_over_ranks(time.perf_counter() - t0, self.device)
        os.makedirs(f'npy/{self.method_name}', exist_ok=True)
        tag = '' if self.world == 1 else f'_rank{self.rank}'
        np.save(f'npy/{self.method_name}/benchmark_init{tag}.npy', bench_init)
        np.save(f'npy/{self.method_name}/benchmark_results{tag}.npy', bench_results)
        D.barrier()
        if self.rank == 0:
            log(f'{self.method_name} benchmark: {n} images on {self.world} GPU(s) in {dt:.2f} s -> npy/{self.method_name}/benchmark_*.npy', self.logfile)
        return bench_init, bench_results


class YONDParser:
    def __init__(self):
        self.parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)

    def parse(self, args=None):
        a = self.parser
        a.add_argument('--runfile', '-f', default="runfiles/YOND/SIDD_simple+full_pre_grumix.yml", type=Path, help="path to config")
        a.add_argument('--mode', '-m', default='eval', type=str, help="eval or test")
        a.add_argument('--debug', action='store_true', default=False)
        a.add_argument('--nofig', action='store_true', default=True, help="kept for CLI compatibility (store_true with default True, as in the reference: it cannot be turned off); --fig turns the figures on")
        a.add_argument('--fig', action='store_true', default=False, help="render the noisy frame, the ground truth and every round's output to sRGB on the GPU: "
                       "PNGs under <result_dir>/<method_name>/ and PSNR(sRGB) / SSIM(sRGB) beside the raw metrics")
        a.add_argument('--nohost', action='store_true', default=False)
        a.add_argument('--gpu', default="0", help="kept for CLI compatibility; ranks pick their device from LOCAL_RANK")
        a.add_argument('--synthetic', type=int, default=40, help="number of synthetic stand-in images when no dataset is found "
                       "(40 = the SIDD validation set's size; each with a 3000 x 5328 frame for the round-1 estimate)")
        a.add_argument('--verbose', action='store_true', default=False)
        a.add_argument('--loaders', type=int, default=4, help="loader threads that read and upload the items ahead of the GPU")
        a.add_argument('--prefetch', type=int, default=4, help="items the loader threads may be ahead of the GPU (at least two groups)")
        a.add_argument('--no-stream', dest='stream', action='store_false', default=True, help="one group at a time instead of consecutive groups overlapped on two HIP streams")
        a.add_argument('--group', type=int, default=4, help="images denoised together: round 1 of a group is ONE batch-(32 x group) forward, round 2 another "
                       "(per image the results are those of --group 1)")
        a.add_argument('--save', choices=('none', 'dn16', 'f32'), default='none', help="keep the denoised frames: the full-frame drivers write every item's last round to "
                       "<result_dir>/<method_name>/<name>.npy (+ .json) as uint16 DN (dn16: digital gain kept) or float32 in [0, 1] (f32); YOND_SIDD eval with f32 "
                       "writes the reference's cache npy/<method_name>/<k:03d>.npy, float32 [max_iter + 1][256][8192]")
        a.add_argument('--host-ingest', dest='host_ingest', action='store_true', default=False, help="full-frame drivers: normalise the raw frames on the host in "
                       "NumPy and upload float32 (the earlier path) instead of uploading the raw DN and normalising on the device")
        a.add_argument('--fit', choices=('lsq', 'ransac'), default=None, help="the line fit of the noise-level estimate: lsq, the reference's shipped least "
                       "squares (default), or ransac, its polyfit(ransac=True) replayed on the GPU (needs scikit-learn for the subset draws; frames are then "
                       "estimated one at a time, outside the device chain).  Overrides the runfile's pipeline.est_fit")
        a.add_argument('--illum-corr', dest='illum_corr', choices=('off', 'frame', 'cfa'), default=None, help="full-frame drivers: the ELD protocol's illuminance "
                       "correction before PSNR / SSIM -- one least-squares gain per frame between the clamped output and the unsaturated ground truth "
                       "(frame), or one per CFA channel (cfa); the corrected metrics are reported beside the plain ones as PSNR(ic) / SSIM(ic).  Overrides "
                       "the runfile's pipeline.illum_corr")
        from .pgnoise import synth_noise_arg
        a.add_argument('--synth-noise', dest='synth_noise', type=synth_noise_arg, default=None, metavar='K,SIGMA', help="full-frame drivers: take every item's clean "
                       "frame (hr if present, else lr) as the ground truth and make the noisy frame on the GPU, Poisson-Gaussian with system gain K and read "
                       "noise SIGMA in DN; the log and the metrics gain the true level and the estimator's relative error per round, both in the estimate's units: "
                       "DN of the frame the pipeline is handed, so a frame of ratio r reports ratio * K and ratio * SIGMA as the truth")
        from .camnoise import camera_noise_arg
        a.add_argument('--camera-noise', dest='camera_noise', type=camera_noise_arg, default=None, metavar='SPEC', help="full-frame drivers: as --synth-noise, "
                       "with the low-light camera noise model instead of Poisson-Gaussian: SPEC is a comma list of key=value in DN at capture (before the "
                       "ratio), e.g. code=pgrq,K=0.22,sigTL=0.76,sigGs=1.26,sigR=0.23,lam=-0.026; code holds the reference's letters (p Poisson shot, "
                       "g Tukey-lambda read noise of scale sigTL and shape lam -- without g Gaussian read noise sigGs --, r row noise sigR, q quantisation, "
                       "d dark bias, b shot only); optional bias=b0/b1/b2/b3, mfm=, clip=none|01|sensor.  The truth reported is the Poisson-Gaussian "
                       "level of the same variance, ratio * K and ratio * sigma_eff.  Not together with --synth-noise")
        from .noisekld import noise_kld_arg
        a.add_argument('--noise-kld', dest='noise_kld', type=noise_kld_arg, default=None, metavar='MODEL', help="full-frame drivers: how well a noise model "
                       "explains every frame's noise -- the KL divergence between the histogram of noisy - clean and the histogram of residuals drawn "
                       "from MODEL on the same clean frame (the reference's cal_kld), reported per frame as KLD, per CFA position, per intensity band, with "
                       "the model's own sampling floor (the model against itself under a second noise key).  MODEL: est (the last round's blind "
                       "estimate), K,SIGMA (Poisson-Gaussian, DN at capture) or cam:<a --camera-noise SPEC>.  Overrides the runfile's pipeline.noise_kld")
        a.add_argument('--kld-range', dest='kld_range', type=float, default=None, metavar='R', help="--noise-kld: 64 bins on [-R, R] between two catch-all "
                       "bins (default 0.1, the reference's edges).  Overrides pipeline.noise_kld_range")
        a.add_argument('--kld-bands', dest='kld_bands', type=int, default=None, metavar='N', help="--noise-kld: split the histograms into N intensity bands of "
                       "the clean frame, thresholds np.linspace(0, 1, N + 1)[1:-1] (default 0: none).  Overrides pipeline.noise_kld_bands")
        from .bpc import bad_pixels_arg, synth_defects_arg
        a.add_argument('--bad-pixels', dest='bad_pixels', type=bad_pixels_arg, default=None, metavar='FILE.npy|auto|auto:T', help="full-frame drivers: repair "
                       "defective pixels before the frame is estimated and denoised -- FILE.npy: the camera's bad-point list, an int [n][2] array of "
                       "(row, col), each replaced by the 3x3 median of its own CFA plane (the reference's repair_bad_pixels); auto: no list, a pixel that "
                       "stands out from all eight same-colour neighbours by T standard deviations (default 6) of a blind noise estimate of the frame is "
                       "repaired (this project's extension; one extra estimate per frame).  Overrides the runfile's pipeline.bad_pixels")
        a.add_argument('--synth-defects', dest='synth_defects', type=synth_defects_arg, default=None, metavar='N[,LEVEL]', help="full-frame drivers, with "
                       "--synth-noise or --camera-noise: N isolated stuck pixels are set in every noisy frame (LEVEL in the frame's units; default: the "
                       "white level, ratio * 1.0), keyed by the item's name; the ground truth stays clean, and with --bad-pixels the log reports how many "
                       "were found and how many detections were false")
        from .rownoise import row_denoise_arg
        a.add_argument('--row-denoise', dest='row_denoise', type=row_denoise_arg, nargs='?', const=row_denoise_arg('on'), default=None, metavar='SPEC',
                       help="full-frame drivers: take row noise (banding) out of every frame before it is estimated and denoised, after --bad-pixels -- "
                       "the reference's row_denoise: the means of the even and of the odd sensor rows are smoothed by a 1-D bilateral filter and "
                       "mean - smoothed is subtracted from the row.  SPEC: empty or on, or sc=10,ss=auto,d=25,per=row|plane (sc: sigma_color in DN at "
                       "capture; ss: sigma_space in rows, auto = 1 + ISO / 200; d: odd diameter up to 63; per=plane: one offset per row of a CFA "
                       "plane, this project's extension).  It assumes smooth row means: on a scene, content leaks into the offsets.  Overrides the "
                       "runfile's pipeline.row_denoise")
        return a.parse_args(args)


def main(argv=None):
    trainer = YOND_SIDD(argv)
    main.trainer = trainer                                   # the last run's driver object (its .metrics, .sample_dir)
    try:
        out = None
        if 'eval' in trainer.mode:                           # YOND_SIDD.py:736-744
            trainer.change_eval_dst('eval')
            out = trainer.eval(-1)
        if 'test' in trainer.mode:
            trainer.change_eval_dst('test')
            out = trainer.benchmark()
        return out
    finally:
        D.finalize()


if __name__ == '__main__':
    main()
