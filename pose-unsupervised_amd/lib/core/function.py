"""Evaluation slice of the reference's core/function.py on the HIP path.

``validate_batch`` is the body of the reference's validation loop
(function.py:555-644) for one batch of V views: forward, optional flip test (mirrored
input folded into the input pack, heatmaps brought back / shifted / averaged by one
posu_flip_back launch per view), weighted-MSE loss, PCK accuracy, and
``get_final_preds`` per view with the predictions interleaved view-minor
(``preds[k::nviews]``) exactly as the reference stores them.  Everything stays on the
device until the final copy of predictions and heatmaps.

With NETWORK.AGGRE the cross-view Aggregation runs too (models.multiview_pose_resnet),
TEST.FUSE_OUTPUT routes the outputs (``fuse_routing``), and the loss carries the
reference's AGGRE terms (function.py:597-609): the consistent loss between the raw and
aggregated heatmaps of the H36M samples (LOSS.USE_CONSISTENT_LOSS, plain mean MSE) and,
with DATASET.PSEUDO_LABEL_PATH, the weighted MSE of the routed outputs against the
pseudo-label targets times LOSS.MSE_LOSS_WEIGHT.

``validate`` keeps the reference signature (function.py:529-536) and its outputs: the
``heatmaps_locations_<subset>_<type>.h5`` file that run/test/test_triangulate.py reads
(keys heatmaps / locations / joint_names_order, u2a-selected joints) and
``dataset.evaluate``'s perf indicator.  Debug-image dumps and tensorboard are not part
of this build.

``train`` keeps the reference signature (function.py:91-92) and runs its step for the losses this
build has.  What the reference's loop reads back every step -- ``loss.item()`` and one ``.item()`` per
loss, ``accuracy`` on host copies of every view's heatmaps, the gradient-norm watch, the boolean-mask
selection of the H36M samples -- stays on the device here (posu_pck_accuracy, posu_grad_row_norms,
posu_meters_update; the selection is decided on the host from ``meta``), so between two log lines
the host only enqueues.

``validate_device`` / ``validate_batch_device`` are the same loop for an epoch that stays on the device:
one posu_decode_views launch per batch does the flip-test merge, the decode and the accuracy of all
views and writes into preallocated epoch buffers in the reference's row order; loss and accuracy meters
live in a device table; the host reads the device only to print and once at the end.  ``validate`` and
``validate_batch`` are unchanged.
"""
import logging
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from core.evaluate import accuracy
from core.inference import get_final_preds
from posu import ops
from utils.transforms import flip_pair_order

logger = logging.getLogger(__name__)


def fuse_routing(raw_features, aggre_features, is_aggre, meta):
    """function.py:33-45: per sample, 3/5 aggregated + 2/5 raw for H36M samples, raw
    otherwise (one masked blend per view on the device)."""
    if not is_aggre:
        return raw_features
    output = []
    for r, a, m in zip(raw_features, aggre_features, meta):
        h36m = torch.tensor([s == 'h36m' for s in m['source']], device=a.device).view(-1, 1, 1, 1)
        output.append(torch.where(h36m, 3 / 5 * a + 2 / 5 * r, r))
    return output


def select_out_h36m(raw_features, aggre_features, meta):
    """function.py:47-61: per view, the raw and aggregated heatmaps of the H36M samples."""
    raw_h36m, agg_h36m = [], []
    for r, a, m in zip(raw_features, aggre_features, meta):
        idx = torch.tensor([s == 'h36m' for s in m['source']], dtype=torch.bool, device=r.device)
        raw_h36m.append(r[idx])
        agg_h36m.append(a[idx])
    return raw_h36m, agg_h36m


def _h36m_rows(m):
    return [i for i, s in enumerate(m['source']) if s == 'h36m']


def _take_rows(t, rows):
    """Rows of a host meta entry (tensor, array or list)."""
    if isinstance(t, torch.Tensor):
        return t[torch.as_tensor(rows, dtype=torch.long)]
    if isinstance(t, np.ndarray):
        return t[np.asarray(rows, dtype=np.int64)]
    return [t[i] for i in rows]


def select_out_h36m_meta(meta, key_list):
    """function.py:62-75: per view the `key_list` entries of the H36M samples (host data, selected on
    the host); [] when the batch has none."""
    new_meta = []
    for m in meta:
        rows = _h36m_rows(m)
        if not rows:
            break
        new_meta.append({key: _take_rows(m[key], rows) for key in key_list})
    assert len(new_meta) == 0 or len(new_meta) == len(meta)
    return new_meta


def percent_of_datasource(meta):
    """function.py:78-88: the share of each data source in the batch, for the log line."""
    sources = list(meta[0]['source'])
    counts = {}
    for s in sources:
        counts[s] = counts.get(s, 0) + 1
    return ''.join('{} {:.1%}\t'.format(k, v / len(sources)) for k, v in counts.items())


class AverageMeter(object):
    """Computes and stores the average and current value (function.py:693-709), on the host; train()
    keeps its per-step meters in a device table (posu_meters_update) and fills these only to print."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


# losses of the reference's loop that this build does not have (core.loss raises when one is built)
UNBUILT_LOSS_FLAGS = ('USE_GLOBAL_MI_LOSS', 'USE_LOCAL_MI_LOSS', 'USE_DOMAIN_TRANSFER_LOSS', 'USE_VIEW_MI_LOSS',
                      'USE_JOINTS_MI_LOSS')
# slots of train()'s device meter table
METERS = ('loss', 'mse', 'acc', 'consistent', 'fund', 'hmi_g', 'hmi_d', 'mse_grad', 'fund_grad', 'hmi_grad')


def _loss_scaler_of(model):
    """The posu.amp.LossScaler an fp16 base model carries (DDP-wrapped or not, multi-view or not)."""
    base = getattr(model, 'module', model)
    for m in (base, getattr(base, 'resnet', None)):
        scaler = getattr(m, 'loss_scaler', None)
        if scaler is not None:
            return scaler
    return None


class _DeviceMeters:
    """The loop's AverageMeters as one [M, 3] f64 device table (val, sum, count), updated by one
    posu_meters_update launch per step and read only to print."""

    def __init__(self, device, names=METERS):
        self.device = device
        self.names = tuple(names)
        self.table = torch.zeros((len(self.names), 3), dtype=torch.float64, device=device)
        self.vals = torch.zeros((len(self.names),), dtype=torch.float64, device=device)
        self._weights = {}
        self._slots = {}

    def weights(self, nsamples):
        """The reference's weights (function.py:376-457): len(input) * N for the loss and MSE meters
        and, at function.py:380, for the consistent meter as well; 1 for the others; the accuracy slot
        is filled per step with the device value cnt."""
        if nsamples not in self._weights:
            w = [float(nsamples) if name in ('loss', 'mse', 'consistent') else 1.0 for name in self.names]
            self._weights[nsamples] = torch.tensor(w, dtype=torch.float64).to(self.device)
        return self._weights[nsamples]

    def _slot_index(self, slots):
        if slots not in self._slots:
            self._slots[slots] = torch.tensor(slots, dtype=torch.long).to(self.device)
        return self._slots[slots]

    def update(self, values, nsamples, acc_weight):
        """values: {meter name: 0-dim device tensor or Python number}; the others keep their state.
        The f32 scalars (the losses) and the f64 ones (accuracy, gradient norms) each reach the value
        vector as one stack and one index_copy_; then one posu_meters_update launch."""
        groups = {torch.float32: ([], []), torch.float64: ([], []), 'host': ([], [])}
        for slot, name in enumerate(self.names):
            v = values.get(name)
            if v is None:
                continue
            key = v.dtype if isinstance(v, torch.Tensor) else 'host'
            if key not in groups:
                v, key = v.double(), torch.float64
            groups[key][0].append(slot)
            groups[key][1].append(v.detach().reshape(()) if key != 'host' else float(v))
        for key, (slots, vs) in groups.items():
            if not slots:
                continue
            if key == 'host':   # a term that was skipped this step (no H36M sample): its Python 0
                stacked = torch.tensor(vs, dtype=torch.float64).to(self.device)
            else:
                stacked = torch.stack(vs).to(torch.float64)
            self.vals.index_copy_(0, self._slot_index(tuple(slots)), stacked)
        w = self.weights(nsamples)
        if acc_weight is not None:
            acc = self.names.index('acc')
            w[acc:acc + 1].copy_(acc_weight.reshape(1))
        ops.meters_update(self.table, self.vals, w, [name in values for name in self.names])

    def read(self):
        """One device-to-host copy -> {name: AverageMeter}."""
        host = self.table.cpu().numpy()
        out = {}
        for name, (val, total, count) in zip(self.names, host):
            m = AverageMeter()
            m.val, m.sum, m.count = float(val), float(total), float(count)
            m.avg = m.sum / m.count if m.count else 0
            out[name] = m
        return out


def train(config, data, model_dict, criterion_dict, optim_dict, epoch, output_dir, writer_dict, rank):
    """function.py:91-527 for the losses of this build: weighted MSE on the raw (and, with AGGRE, the
    routed) outputs, the consistent loss, FundamentalLoss, HeatmapMILoss (discriminator steps on even
    epochs, the generator term on odd ones) and the gradient-norm watch, then the optimiser step (through
    the base model's posu.amp.LossScaler when it has one).  PCK accuracy, the watch and the running meters
    stay on the device: on a step with i % PRINT_FREQ != 0 nothing is read back and nothing synchronises.
    Returns {meter name: {'val', 'avg', 'sum', 'count'}} read once after the last step (rank 0; {} on
    the other ranks).  Debug images are not written."""
    from core.evaluate import accuracy_device
    from utils.gradients import check_grad_norm
    from utils.transforms import generate_integral_preds_2d_th, transform_back_th
    L = config.LOSS
    for flag in UNBUILT_LOSS_FLAGS:
        if getattr(L, flag, False):
            raise NotImplementedError('train: LOSS.%s is set, and that loss is not part of this build' % flag)
    device = torch.device('cuda', rank)
    is_aggre = bool(config.NETWORK.AGGRE)
    fuse = is_aggre and bool(getattr(config.TEST, 'FUSE_OUTPUT', False))
    use_cons = bool(getattr(L, 'USE_CONSISTENT_LOSS', False))
    use_fund = bool(getattr(L, 'USE_FUNDAMENTAL_LOSS', False))
    use_hmi = bool(getattr(L, 'USE_HEATMAP_MI_LOSS', False))
    watch = bool(getattr(L, 'WATCH_GRAD_NORM', False))
    hmi_generator = use_hmi and epoch % 2 != 0
    mse_crit = criterion_dict['mse_weights']
    base_model = model_dict['base_model']
    base_opt = optim_dict['base_model']
    scaler = _loss_scaler_of(base_model)
    batch_time, data_time = AverageMeter(), AverageMeter()
    meters = _DeviceMeters(device) if rank == 0 else None

    for model in model_dict.values():
        model.train()

    end = time.time()
    for i, (input, target, weight, meta) in enumerate(data):
        data_time.update(time.time() - end)
        input = [view.to(device, non_blocking=False) for view in input]
        nsamples = len(input) * input[0].size(0)
        raw_features, aggre_features, low_features, high_features = base_model(input)
        output = fuse_routing(raw_features, aggre_features, is_aggre, meta) if fuse else raw_features

        step_vals = {}
        loss = 0
        mse_loss = 0
        target_cuda = [t.to(device, non_blocking=False) for t in target]
        weight_cuda = [w.to(device, non_blocking=False) for w in weight]
        for t, w, r in zip(target_cuda, weight_cuda, raw_features):
            mse_loss = mse_loss + mse_crit(r, t, w) * L.MSE_LOSS_WEIGHT
        loss = loss + mse_loss
        if is_aggre:   # function.py:185-188, as written there: mse_loss is added to the loss again
            for t, w, o in zip(target_cuda, weight_cuda, output):
                mse_loss = mse_loss + mse_crit(o, t, w) * L.MSE_LOSS_WEIGHT
            loss = loss + mse_loss

        if use_hmi:    # function.py:259-278
            joint_idx = config.HEATMAP_DISCRIMINATOR.JOINT_IDX
            if not hmi_generator:
                hmi_loss_d = criterion_dict['heatmap_mi'].views([l.detach() for l in low_features],
                                                                [o.detach() for o in output], weight_cuda, meta,
                                                                joint_idx=joint_idx)
                optim_dict['heatmap_discriminator'].zero_grad()
                hmi_loss_d.backward()
                optim_dict['heatmap_discriminator'].step()
                step_vals['hmi_d'] = hmi_loss_d
            else:
                hmi_loss_g = criterion_dict['heatmap_mi'].views(low_features, output, weight_cuda, meta,
                                                                joint_idx=joint_idx) * L.HEATMAP_MI_LOSS_WEIGHT
                loss = loss + hmi_loss_g
                step_vals['hmi_g'] = hmi_loss_g

        # the H36M samples, chosen on the host from meta (no boolean-mask indexing: that is a nonzero
        # and a synchronisation); every view selects by its own meta, like select_out_h36m
        consistent_loss = 0
        fund_loss = 0
        rows = [_h36m_rows(m) for m in meta]
        have_h36m = len(rows[0]) != 0
        if (use_fund or (is_aggre and use_cons)) and have_h36m:
            # one index upload per view and step; None: every sample of the view is H36M
            index = [None if len(r) == len(m['source']) else torch.tensor(r, dtype=torch.long).to(device)
                     for r, m in zip(rows, meta)]

            def pick(tensors):
                return [t if k is None else t.index_select(0, k) for t, k in zip(tensors, index)]
            s_raw = pick(raw_features)
            s_weight, s_output = pick(weight_cuda), pick(output)
            s_meta = select_out_h36m_meta(meta, ['center', 'scale', 'subject'])
            assert len(s_weight[0]) == len(s_output[0]) == len(s_raw[0])
            if is_aggre and use_cons:   # function.py:291-296
                cal_loss = criterion_dict['mse'](torch.cat(s_raw, dim=0), torch.cat(pick(aggre_features), dim=0))
                loss = loss + cal_loss * L.CONSISTENT_LOSS_WEIGHT
                consistent_loss = cal_loss.detach().double() * L.CONSISTENT_LOSS_WEIGHT
            if use_fund:                # function.py:299-310
                joints2d_list = transform_back_th(config, [generate_integral_preds_2d_th(o) for o in s_output],
                                                  s_meta)
                fund_loss = criterion_dict['fundamental'](joints2d_list, s_weight, s_meta) * L.FUNDAMENTAL_LOSS_WEIGHT
                loss = loss + fund_loss

        if watch and have_h36m:         # function.py:352-362
            losses_dict = OrderedDict([('mse', mse_loss)])
            if use_fund:
                losses_dict['fund'] = fund_loss
            if hmi_generator:
                losses_dict['hmi_g'] = hmi_loss_g
            grad_dict = check_grad_norm(losses_dict, raw_features, norm=1)
            for name, value in grad_dict.items():
                step_vals[{'mse': 'mse_grad', 'fund': 'fund_grad', 'hmi_g': 'hmi_grad'}[name]] = value

        base_opt.zero_grad()
        if scaler is not None:
            scaler.scale(loss).backward()
            scaler.step(base_opt)
            scaler.update()
        else:
            loss.backward()
            base_opt.step()

        if rank == 0:
            step_vals['loss'] = loss
            step_vals['mse'] = mse_loss
            if use_cons:
                step_vals['consistent'] = consistent_loss
            if use_fund:
                step_vals['fund'] = fund_loss
            _, _, _, _, acc_step = accuracy_device(output, target_cuda)
            step_vals['acc'] = acc_step[0]
            meters.update(step_vals, nsamples, acc_step[1])
            batch_time.update(time.time() - end)
            end = time.time()

            if i % config.PRINT_FREQ == 0:
                m = meters.read()       # the one read between two log lines
                msg = 'Epoch: [{0}][{1}/{2}]\t' \
                      'Time {batch_time.val:.3f}s ({batch_time.avg:.3f}s)\t' \
                      'Speed {speed:.1f} samples/s\t' \
                      'Data {data_time.val:.3f}s ({data_time.avg:.3f}s)\t' \
                      'Memory {memory:.1f}\t' \
                      'Loss {loss.val:.5f} ({loss.avg:.5f})\t' \
                      'MSE Loss {mse_loss.val:.4f} ({mse_loss.avg:.4f})\t' \
                      'Accuracy {acc.val:.3f} ({acc.avg:.3f})\t'.format(
                          epoch, i, len(data), batch_time=batch_time, speed=nsamples / batch_time.val,
                          data_time=data_time, loss=m['loss'], acc=m['acc'],
                          memory=torch.cuda.memory_allocated(0), mse_loss=m['mse'])
                if use_cons:
                    msg += 'Consistent Loss {cons_loss.val:.5f} ({cons_loss.avg:.5f})\t'.format(cons_loss=m['consistent'])
                if use_fund:
                    msg += 'Fundamental Loss {fund_loss.val:.4f} ({fund_loss.avg:.4f})\t'.format(fund_loss=m['fund'])
                if use_hmi:
                    msg += 'Hmi_g Loss {hmi_loss_g.val:.4f} ({hmi_loss_g.avg:.4f})\t' \
                           'Hmi_d Loss {hmi_loss_d.val:.4f} ({hmi_loss_d.avg:.4f})\t'.format(
                               hmi_loss_g=m['hmi_g'], hmi_loss_d=m['hmi_d'])
                if watch:
                    msg += 'MSE_grad Norm {mse_grad_norm.val:.6f} ({mse_grad_norm.avg:.6f})\t'.format(
                        mse_grad_norm=m['mse_grad'])
                    if use_fund:
                        msg += 'Fund_grad Norm {fund_grad_norm.val:.4f} ({fund_grad_norm.avg:.4f})\t'.format(
                            fund_grad_norm=m['fund_grad'])
                    if hmi_generator:
                        msg += 'Hmi_grad Norm {hmi_grad_norm.val:.5f} ({hmi_grad_norm.avg:.5f})\t'.format(
                            hmi_grad_norm=m['hmi_grad'])
                msg += percent_of_datasource(meta)
                logger.info(msg)

                if writer_dict is not None:
                    writer = writer_dict['writer']
                    global_steps = writer_dict['train_global_steps']
                    writer.add_scalar('train_loss', m['loss'].val, global_steps)
                    writer.add_scalar('train_mse_loss', m['mse'].val, global_steps)
                    writer.add_scalar('train_acc', m['acc'].val, global_steps)
                    writer_dict['train_global_steps'] = global_steps + 1
                    if use_cons:
                        writer.add_scalar('train_consistent_loss', m['consistent'].val, global_steps)
                    if use_fund:
                        writer.add_scalar('train_fundamental_loss', m['fund'].val, global_steps)
                    if use_hmi:
                        writer.add_scalar('train_hmi_loss_d', m['hmi_d'].val, global_steps)
                        writer.add_scalar('train_hmi_loss_g', m['hmi_g'].val, global_steps)

    if meters is None:
        return {}
    return {name: {'val': m.val, 'avg': m.avg, 'sum': m.sum, 'count': m.count} for name, m in meters.read().items()}


def _run_model(model, views, hflip):
    """model(views) -> (per-view heatmaps, aggregated heatmaps or []); the flip test's
    mirrored input is packed by the HIP input-pack kernel when the model is this build's."""
    base = getattr(model, 'module', model)          # DDP-wrapped or not
    resnet = getattr(base, 'resnet', None)
    if hflip and resnet is not None and hasattr(resnet, 'plan') and not resnet.training:
        plan = resnet.plan(views[0].device)
        hm, _, _ = plan.run(plan.pack_input(views, hflip=True), keep_features=False)
        raw = list(torch.split(hm, views[0].shape[0], dim=0))
        agg = base.aggre_layer(raw) if getattr(base, 'aggre_layer', None) is not None else []
        return raw, agg
    if hflip:
        views = [torch.flip(v, dims=[3]) for v in views]
    raw, agg, _, _ = model(views)
    return raw, agg


def validate_batch(config, model, input, target=None, weight=None, meta=None, flip_pairs=None,
                   criterion=None, criterion_dict=None):
    """One batch of the reference's validate loop.

    input: V x [N, 3, H, W] cuda f32; target / weight: V x [N, J, h, w] / [N, J, 1] (optional);
    meta: V dicts with 'center', 'scale' ([N, 2]).  Returns a dict with
    output (V x [N, J, h, w] cuda), preds ([V*N, J, 3] numpy, row k::V = view k), heatmaps
    ([V*N, J, h, w] numpy, same order), loss (float or None), acc / cnt (or None)."""
    device = input[0].device
    nviews = len(input)
    fuse = bool(config.NETWORK.AGGRE) and bool(getattr(config.TEST, 'FUSE_OUTPUT', False))
    with torch.no_grad():
        raw, agg = _run_model(model, input, False)
        output = fuse_routing(raw, agg, fuse, meta) if fuse else raw
        if config.TEST.FLIP_TEST:
            raw_f, agg_f = _run_model(model, input, True)
            flipped = fuse_routing(raw_f, agg_f, fuse, meta) if fuse else raw_f
            perm = torch.tensor(flip_pair_order(output[0].shape[1], flip_pairs or []), dtype=torch.int32,
                                device=device)
            output = [ops.flip_back(f, perm, hm=o, shift=bool(config.TEST.SHIFT_HEATMAP))
                      for o, f in zip(output, flipped)]
        res = {'output': output, 'loss': None, 'acc': None, 'cnt': None}
        if target is not None:
            target = [t.to(device) for t in target]
            criterion = criterion or (criterion_dict or {}).get('mse_weights')
            if criterion is not None and weight is not None:
                weight = [w.to(device) for w in weight]
                loss = 0
                for t, w, r in zip(target, weight, raw):   # on the raw outputs (function.py:589-595)
                    loss = loss + criterion(r, t, w)
                if config.NETWORK.AGGRE:                   # function.py:597-609
                    if getattr(config.LOSS, 'USE_CONSISTENT_LOSS', False):
                        raw_h36m, agg_h36m = select_out_h36m(raw, agg, meta)
                        assert len(raw_h36m[0]) == len(agg_h36m[0])
                        if len(raw_h36m[0]) != 0:
                            rh, ah = torch.cat(raw_h36m, dim=0), torch.cat(agg_h36m, dim=0)
                            # torch.nn.MSELoss(reduction='mean') = the joints MSE (a sum of
                            # per-joint means) / J, on the HIP reduction kernel
                            loss = loss + ops.joints_mse(rh.contiguous(), ah.contiguous(), None) / rh.shape[1]
                    if getattr(config.DATASET, 'PSEUDO_LABEL_PATH', ''):
                        for t, w, o in zip(target, weight, output):
                            loss = loss + criterion(o, t, w) * config.LOSS.MSE_LOSS_WEIGHT
                res['loss'] = float(loss)
            accs, cnts = [], []
            for o, t in zip(output, target):
                _, a, c, _ = accuracy(o, t)
                accs.append(a)
                cnts.append(c)
            res['acc'], res['cnt'] = float(np.mean(accs)), float(np.mean(cnts))
        n = input[0].shape[0]
        njoints, h, w = output[0].shape[1:]
        preds = torch.empty((nviews * n, njoints, 3), dtype=torch.float32, device=device)
        hms = torch.empty((nviews * n, njoints, h, w), dtype=torch.float32, device=device)
        for k, (o, m) in enumerate(zip(output, meta)):
            center = m['center'].numpy() if hasattr(m['center'], 'numpy') else np.asarray(m['center'])
            scale = m['scale'].numpy() if hasattr(m['scale'], 'numpy') else np.asarray(m['scale'])
            p, mv = get_final_preds(config, o, center, scale)
            preds[k::nviews, :, 0:2] = p
            preds[k::nviews, :, 2:3] = mv
            hms[k::nviews] = o
        res['preds'] = preds.cpu().numpy()
        res['heatmaps'] = hms.cpu().numpy()
    return res


def save_heatmaps_locations(file_name, all_heatmaps, all_preds, u):
    """The validate() output file (function.py:671-676) read by test_triangulate.py."""
    try:
        import h5py
    except ImportError as e:  # not installed in this image; the format needs it
        raise ImportError('writing %s needs h5py (the reference writes HDF5 here)' % file_name) from e
    with h5py.File(file_name, 'w') as f:
        f['heatmaps'] = all_heatmaps[:, u, :, :]
        f['locations'] = all_preds[:, u, :]
        f['joint_names_order'] = u


def validate(config, loader, dataset, model_dict, criterion_dict, output_dir, writer_dict, rank):
    """function.py:529-690 without debug images: returns dataset.evaluate's perf indicator."""
    device = torch.device('cuda', rank)
    for model in model_dict.values():
        model.eval()
    nsamples = len(dataset) * 4
    njoints = config.NETWORK.NUM_JOINTS
    height = int(config.NETWORK.HEATMAP_SIZE[0])
    width = int(config.NETWORK.HEATMAP_SIZE[1])
    all_preds = np.zeros((nsamples, njoints, 3), dtype=np.float32)
    all_heatmaps = np.zeros((nsamples, njoints, height, width), dtype=np.float32)
    idx = 0
    end = time.time()
    for i, (input, target, weight, meta) in enumerate(loader):
        input = [view.to(device, non_blocking=False) for view in input]
        r = validate_batch(config, model_dict['base_model'], input, target, weight, meta,
                           flip_pairs=getattr(dataset, 'flip_pairs', None), criterion_dict=criterion_dict)
        nimgs = r['preds'].shape[0]
        all_preds[idx:idx + nimgs] = r['preds']
        all_heatmaps[idx:idx + nimgs] = r['heatmaps']
        idx += nimgs
        if i % config.PRINT_FREQ == 0 and rank == 0:
            logger.info('Test: [%d/%d]\tTime %.3f\tLoss %s\tAccuracy %s', i, len(loader), time.time() - end,
                        r['loss'], r['acc'])
        end = time.time()
    perf_indicator = 1000
    if rank == 0:
        u2a = {k: v for k, v in dataset.u2a_mapping.items() if v != '*'}
        u = np.array([m[0] for m in sorted(u2a.items(), key=lambda x: x[0])])
        file_name = os.path.join(output_dir, 'heatmaps_locations_%s_%s.h5' % (dataset.subset, dataset.dataset_type))
        save_heatmaps_locations(file_name, all_heatmaps, all_preds, u)
        _, perf_indicator = dataset.evaluate(all_preds[:, u, :],
                                             output_dir if config.DEBUG.SAVE_ALL_PREDS else None)
    return perf_indicator


# slots of validate_device()'s device meter table (losses / avg_acc of function.py:542-543)
VALID_METERS = ('loss', 'acc')


def validate_batch_device(config, model, input, target, weight, meta, flip_pairs, criterion_dict, preds_out,
                          heatmaps_out, row0):
    """``validate_batch`` for an epoch that stays on the device: the same model runs, ``fuse_routing`` and loss
    terms in the same order with the same ops, then one ``ops.decode_views`` call in place of the per-view
    flip-back, accuracy and ``get_final_preds`` calls.

    input: V x [N, 3, H, W] cuda; target / weight: V x [N, J, h, w] / [N, J, 1] (host or cuda); meta: V dicts with
    host 'center', 'scale' ([N, 2]) and, for the AGGRE terms, 'source'.  preds_out [R, J, 3] f32 cuda and
    heatmaps_out ([R, J, h, w] f32 cuda, or None: the merged heatmaps are not stored) are the epoch's buffers;
    rows row0 + n * V + v are written, so that ``preds_out[row0 + k:row0 + V * N:V]`` is view k
    (``preds[k::nviews]``).  Returns a dict of device tensors only: loss (0-dim f32), acc and cnt (0-dim f64:
    the means over the views, what ``validate_batch`` returns as floats), acc_table ([V, J + 1] f64), output
    (the V routed outputs before the flip-test merge) and rows (V * N).  Nothing is read from the device: the
    H36M rows of the consistent loss are chosen on the host from ``meta``."""
    from utils.transforms import batch_inverse_affines
    device = input[0].device
    nviews = len(input)
    fuse = bool(config.NETWORK.AGGRE) and bool(getattr(config.TEST, 'FUSE_OUTPUT', False))
    criterion = criterion_dict['mse_weights']
    with torch.no_grad():
        raw, agg = _run_model(model, input, False)
        output = fuse_routing(raw, agg, fuse, meta) if fuse else raw
        flipped = perm = None
        if config.TEST.FLIP_TEST:
            raw_f, agg_f = _run_model(model, input, True)
            flipped = fuse_routing(raw_f, agg_f, fuse, meta) if fuse else raw_f
            perm = torch.tensor(flip_pair_order(output[0].shape[1], flip_pairs or []), dtype=torch.int32).to(device)
        target = [t.to(device) for t in target]
        weight = [w.to(device) for w in weight]
        loss = 0
        for t, w, r in zip(target, weight, raw):   # on the raw outputs (function.py:589-595)
            loss = loss + criterion(r, t, w)
        if config.NETWORK.AGGRE:                   # function.py:597-609
            if getattr(config.LOSS, 'USE_CONSISTENT_LOSS', False):
                rows = [_h36m_rows(m) for m in meta]
                if len(rows[0]) != 0:
                    # select_out_h36m's rows through an index made on the host: a boolean mask is a nonzero
                    # and a synchronisation
                    index = [torch.tensor(r, dtype=torch.long).to(device) for r in rows]
                    rh = torch.cat([r.index_select(0, k) for r, k in zip(raw, index)], dim=0)
                    ah = torch.cat([a.index_select(0, k) for a, k in zip(agg, index)], dim=0)
                    assert rh.shape[0] == ah.shape[0]
                    loss = loss + ops.joints_mse(rh.contiguous(), ah.contiguous(), None) / rh.shape[1]
            if getattr(config.DATASET, 'PSEUDO_LABEL_PATH', ''):
                for t, w, o in zip(target, weight, output):
                    loss = loss + criterion(o, t, w) * config.LOSS.MSE_LOSS_WEIGHT
        h, w_ = output[0].shape[2], output[0].shape[3]
        trans = np.concatenate([batch_inverse_affines(np.asarray(m['center']), np.asarray(m['scale']), [w_, h])
                                for m in meta], axis=0)       # [V * N, 2, 3] f64, view-major: one upload
        T = torch.from_numpy(np.ascontiguousarray(trans, dtype=np.float64)).to(device)
        _, _, acc, _, _, step = ops.decode_views(
            output, flipped=flipped, perm=perm, shift=bool(config.TEST.SHIFT_HEATMAP), targets=target, affine64=T,
            post_process=bool(config.TEST.POST_PROCESS), preds_out=preds_out, merged_out=heatmaps_out, row0=row0)
    return {'loss': loss, 'acc': step[0], 'cnt': step[1], 'acc_table': acc, 'output': output,
            'rows': nviews * input[0].shape[0]}


class ValidationResult:
    """What ``validate_device`` leaves: perf_indicator and name_values (``dataset.evaluate``'s; 1000 and None on
    the other ranks), locations ([nsamples, J, 3] f32 cuda: x, y, maxval per union joint), heatmaps
    ([nsamples, J, h, w] f32 cuda, or None), u (the annotated union joints, sorted) and meters
    ({'loss' / 'acc': {'val', 'avg', 'sum', 'count'}}, read once after the last batch)."""

    def __init__(self, perf_indicator, name_values, locations, heatmaps, u, meters):
        self.perf_indicator = perf_indicator
        self.name_values = name_values
        self.locations = locations
        self.heatmaps = heatmaps
        self.u = u
        self.meters = meters


def validate_device(config, loader, dataset, model_dict, criterion_dict, output_dir, writer_dict, rank,
                    keep_heatmaps=True):
    """function.py:529-690 without debug images, with the epoch on the device.  The predictions (and, with
    ``keep_heatmaps``, the heatmaps) of every batch go straight into buffers allocated once at
    len(dataset) * nviews rows; the loss meter (weighted by the batch's images) and the accuracy meter (weighted
    by the device value cnt) live in a device table that is read only on the ``i % PRINT_FREQ == 0`` line and
    once after the last batch.  Between two log lines the host only enqueues.

    With ``keep_heatmaps=True`` the end of the loop is ``validate``'s: one copy to the host, the
    ``heatmaps_locations_<subset>_<type>.h5`` file, ``dataset.evaluate(all_preds[:, u, :], ...)``.  With
    ``keep_heatmaps=False`` no heatmap is stored and no h5 file is written: only the predictions
    ([nsamples, J, 3]) are copied for ``dataset.evaluate``.  Returns a ``ValidationResult``;
    ``result.locations[:, result.u]`` is the cuda ``locations`` tensor that
    ``multiviews.pseudo_label.pseudo_label_round`` takes."""
    device = torch.device('cuda', rank)
    for model in model_dict.values():
        model.eval()
    njoints = config.NETWORK.NUM_JOINTS
    height = int(config.NETWORK.HEATMAP_SIZE[0])
    width = int(config.NETWORK.HEATMAP_SIZE[1])
    all_preds = all_heatmaps = None
    meters = _DeviceMeters(device, names=VALID_METERS)
    idx = 0
    end = time.time()
    for i, (input, target, weight, meta) in enumerate(loader):
        input = [view.to(device, non_blocking=False) for view in input]
        if all_preds is None:                        # the epoch buffers, once the number of views is known
            nsamples = len(dataset) * len(input)
            all_preds = torch.zeros((nsamples, njoints, 3), dtype=torch.float32, device=device)
            if keep_heatmaps:
                all_heatmaps = torch.zeros((nsamples, njoints, height, width), dtype=torch.float32, device=device)
        r = validate_batch_device(config, model_dict['base_model'], input, target, weight, meta,
                                  getattr(dataset, 'flip_pairs', None), criterion_dict, all_preds, all_heatmaps, idx)
        nimgs = r['rows']
        meters.update({'loss': r['loss'], 'acc': r['acc']}, nimgs, r['cnt'])
        idx += nimgs
        if i % config.PRINT_FREQ == 0 and rank == 0:
            m = meters.read()                        # the one read between two log lines
            logger.info('Test: [%d/%d]\tTime %.3f\tLoss %.4f (%.4f)\tAccuracy %.3f (%.3f)', i, len(loader),
                        time.time() - end, m['loss'].val, m['loss'].avg, m['acc'].val, m['acc'].avg)
        end = time.time()
    if all_preds is None:                            # an empty loader
        all_preds = torch.zeros((0, njoints, 3), dtype=torch.float32, device=device)
        all_heatmaps = torch.zeros((0, njoints, height, width), dtype=torch.float32, device=device) \
            if keep_heatmaps else None
    final = {name: {'val': m.val, 'avg': m.avg, 'sum': m.sum, 'count': m.count} for name, m in meters.read().items()}
    u2a = {k: v for k, v in dataset.u2a_mapping.items() if v != '*'}
    u = np.array([m[0] for m in sorted(u2a.items(), key=lambda x: x[0])])
    perf_indicator, name_values = 1000, None
    if rank == 0:
        host_preds = all_preds.cpu().numpy()
        if keep_heatmaps:
            file_name = os.path.join(output_dir, 'heatmaps_locations_%s_%s.h5' % (dataset.subset, dataset.dataset_type))
            save_heatmaps_locations(file_name, all_heatmaps.cpu().numpy(), host_preds, u)
        name_values, perf_indicator = dataset.evaluate(host_preds[:, u, :],
                                                       output_dir if config.DEBUG.SAVE_ALL_PREDS else None)
    return ValidationResult(perf_indicator, name_values, all_preds, all_heatmaps, u, final)
