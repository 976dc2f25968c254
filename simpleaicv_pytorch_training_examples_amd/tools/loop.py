"""The one training-epoch engine and the one timed evaluation pass behind every train_* / test_* / validate_* function of tools/.

  begin_training     model.train(), device, autocast of the loop, the `use_amp: ..., amp_type: ...!` line
  run_epoch          the per-iteration state machine; a train_* function describes its task as a `step_fn` over it
  timed_eval_pass    EMA switch, eval(), no_grad, the two synchronisation points, data / batch time per image
  for_all_datasets   per-dataset evaluation -> `..._for_all_dataset`

Loop semantics are the reference's -- skip a batch when ANY rank saw inf/nan input or a zero/inf/nan loss,
gradient accumulation with `no_sync()`, optional clipping, GradScaler step/update, EMA, mean-
over-ranks loss meter, per-iteration scheduler on the fractional epoch, identical log lines --
but the reference's four host synchronisations and the barrier per iteration (C5-C7 in
SURVEY.md section 2.4) collapse into ONE small all-reduce whose result the host reads a few
iterations late:
  * the skip decision is taken on the device: the flag is all-reduced and handed to the fused
    optimizer kernel as `found_inf`, which then leaves parameters and optimizer state untouched
    (what `optimizer.zero_grad(); continue` achieves in the reference);
  * the loss meter, the "skip this batch!" log line and the iteration counter are updated when
    the (flag, loss, terms...) vector of an iteration is popped from a short queue (`config.host_sync_lag`
    iterations later, default 2; 0 restores a blocking read every iteration), so the host never
    stalls the HIP stream.
"""
import collections
import functools
import time

import torch
import torch.distributed as dist
from torch.amp.autocast_mode import autocast

from ..SimpleAICV.classification.common import AverageMeter, get_amp_type


def _device_of(model):
    return next(model.parameters()).device


def _dist_on(group=None):
    return dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1


def all_reduce_sum_packed(packed, model, group):
    """SUM over the ranks of a small fp32 device tensor (skip flag + loss terms), in place.  With the engine's DDP wrapper on
    RCCL it travels on the SAME communicator and communication stream as the gradient buckets (saicv_comm_*), so the step
    never has collectives of two communicators in flight at once; otherwise torch.distributed carries it."""
    if not _dist_on(group):
        return packed
    comm = getattr(model, 'comm', None)
    if comm is not None and packed.dtype == torch.float32 and packed.is_contiguous():
        comm.allreduce_now(packed, average=False)
    else:
        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    return packed


def all_ranks_agree(mine, config):
    """True iff `mine` is true on EVERY rank of config.group -- a host-side decision made the same way everywhere.  The DETR loop
    leaves the captured step for a batch whose images carry more boxes than config.max_annots (graph_inputs -> None); under DDP one
    rank running the eager step (host-side assignment, eagerly issued bucket all-reduces) while the others replay the graph (captured
    collectives) is two different collective sequences: a hang.  The flag travels over a gloo group (created once per
    config, by every rank at the same iteration): no device synchronisation, ~0.1 ms of host time against a 23 ms step."""
    world = int(getattr(config, 'gpus_num', 1) or 1)
    if world <= 1 or not (dist.is_available() and dist.is_initialized()):
        return bool(mine)
    group = getattr(config, '_saicv_host_group', None)
    if group is None:
        own = getattr(config, 'group', None)
        group = own if dist.get_backend(own) == 'gloo' else dist.new_group(backend='gloo')
        config._saicv_host_group = group
    flag = torch.tensor([1 if mine else 0], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group if group is not None else dist.group.WORLD)
    return bool(int(flag[0]))


def begin_training(model, logger, config):
    """What every train_* function does first -> (device, amp): `with amp():` is the loop's autocast (off unless config.use_amp)."""
    model.train()
    device = _device_of(model)
    amp_type = get_amp_type(model)
    if config.local_rank == 0 and getattr(config, 'total_rank', 0) == 0:
        logger.info(f'use_amp: {config.use_amp}, amp_type: {amp_type}!')
    return device, functools.partial(autocast, device_type=device.type, dtype=amp_type, enabled=bool(config.use_amp))


def run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, total_name, iter_width,
              graph_inputs=None, log_terms=True, term_names=None, chained_total=False, before_step=None, ema=True):
    """One training epoch.  `step_fn(data)` runs forward + criterion under the caller's autocast and returns
    (bad-input flag tensor, loss, batch size); the loss is {name: tensor} or a bare scalar tensor.  Everything else --
    accumulation, the single packed all-reduce of [skip, total, terms...], device-side skip, clipping, scaler, EMA, scheduler,
    lagged host reads and the reference log line -- is here, once.

    A bare scalar makes the packed vector [skip, loss]: no terms vector is built and no finiteness check of terms is launched
    (the captured ResNet-50 / ViT step).  For a dict the terms are logged after the total -- `log_terms=False` leaves them out --
    in the order of `term_names`, or in the dict's own order, learnt on the first forward.  The total of up to four terms is a
    chain of adds; above four (DETR: 18) one stack + one sum instead of a chain of adds and a second stack, d loss / d term
    being 1 either way, unless the caller states `chained_total`.  `ema=False`: the loop has no EMA model whatever the config says.

    config.use_step_graph + `graph_inputs(data) -> tuple of device tensors`: the WHOLE iteration -- forward, criterion, backward
    with its bucket all-reduces, unscale / clip / fused optimizer step, zero_grad, EMA -- is captured once into a hipGraph and
    replayed (engine.StepGraph): the host then issues one graph launch instead of ~700 kernel launches, and `step_fn` is called
    with that tuple.  Only for steps without host reads and with static shapes (drop_last loaders), and accumulation_steps == 1;
    everything the host changes per iteration (the scheduler's learning rates) reaches the captured kernels through the
    optimizer's device table.  `graph_inputs` may return None for a batch that does not fit the captured shapes -- with
    `graph_inputs.may_decline` set, every rank then takes the eager step (all_ranks_agree).  Members of the tuple that are not
    tensors are host values a capture freezes (where the host decides the SHAPE of a batch's step): they are part of the graph's
    key, one graph per combination.  `before_step()` runs on the host before every step, outside any graph.  Graphs live in
    config._saicv_step_graphs, keyed (id(model), id(optimizer), *host values), and serve later epochs."""
    losses = AverageMeter()
    main = config.local_rank == 0 and getattr(config, 'total_rank', 0) == 0
    iters = len(train_loader.dataset) // config.batch_size
    iter_index = 1
    acc_steps = config.accumulation_steps
    assert acc_steps >= 1, 'illegal accumulation_steps!'
    lag = getattr(config, 'host_sync_lag', 2)
    scaler = getattr(config, 'scaler', None) if config.use_amp else None
    clip_norm = getattr(config, 'clip_max_norm', 0) or 0
    clip_value = getattr(config, 'clip_grad_value', 0) or 0
    pending = collections.deque()      # (packed [skip, loss, terms...] device tensor, batch size, log line or None)
    carried_bad = None                 # skip flag of earlier micro-steps of this accumulation window
    # names of the loss terms.  A cached step graph (below) replays WITHOUT running forward_backward again, so learnt names live in
    # a list that is cached with the graph: a second epoch in the same process reuses both (a per-call `keys = None`
    # stayed None from epoch 2 on and the first logged iteration raised on rank 0)
    names = list(term_names or ())

    def drain(keep):
        nonlocal iter_index
        while len(pending) > keep:
            packed, n, log_fmt = pending.popleft()
            vals = packed.tolist()
            if vals[0]:
                if main:
                    logger.info('skip this batch!')
                iter_index -= 1            # the reference does not count a skipped iteration
                continue
            loss = vals[1] / float(config.gpus_num)
            losses.update(loss, n)
            if log_fmt is not None and main:
                terms = ''.join(f'{k}: {v / float(config.gpus_num) * acc_steps:.4f}, ' for k, v in zip(names, vals[2:]))
                logger.info(log_fmt.format(loss=loss * acc_steps) + (terms if log_terms else ''))

    def forward_backward(data, boundary):
        """forward, criterion, (scaled) backward; -> (packed [skip, total / acc_steps, terms...] reduced over the ranks, batch size)"""
        bad, loss_value, n = step_fn(data)
        terms = None
        # the device-side replacement of the reference's isinf / isnan python branches
        if torch.is_tensor(loss_value):
            loss = loss_value
            bad = bad | (loss == 0.) | ~torch.isfinite(loss)
        else:
            if not names:
                names.extend(loss_value.keys())
            if len(names) > 4 and not chained_total:
                stacked = torch.stack([loss_value[k].float() for k in names])
                loss = stacked.sum()
                terms = stacked.detach() / acc_steps
            else:
                loss = sum(loss_value.values())
                terms = torch.stack([loss_value[k].detach().float() for k in names]) / acc_steps
            bad = bad | (loss == 0.) | ~torch.isfinite(loss) | ~torch.isfinite(terms).all()
        loss = loss / acc_steps
        scaled = scaler.scale(loss) if scaler is not None else loss
        if boundary:
            scaled.backward()
        else:
            with model.no_sync():       # no gradient exchange on non-boundary micro-steps
                scaled.backward()
        # one tiny all-reduce carries the skip flag (any rank) and the loss and its terms (sum over ranks)
        packed = torch.stack([bad.float(), loss.detach().float()])
        if terms is not None:
            packed = torch.cat([packed, terms])
        all_reduce_sum_packed(packed, model, config.group)
        return packed, n

    def update(packed):
        """gradient sync wait, inf/nan check, unscale + clip, fused optimizer step, scaler update, zero_grad, EMA"""
        if hasattr(model, 'finish_gradient_sync'):
            model.finish_gradient_sync()
        skip_flag = packed[0:1]
        if getattr(config, 'skip_inf_nan_grad', False) or scaler is not None:
            optimizer.check_finite()
            skip_flag = torch.maximum(skip_flag, optimizer.found_inf)
        inv_scale = scaler.state[2:3] if scaler is not None else None
        if clip_value > 0:             # reference order: unscale, clamp every gradient element, then the norm clip
            optimizer.clip_grad_value_(clip_value, inv_scale)
            inv_scale = None
        if clip_norm > 0:
            optimizer.clip_grad_norm_(clip_norm, inv_scale)
            inv_scale = None
        optimizer.step(inv_scale, skip_flag)
        if scaler is not None:
            scaler._found_inf = optimizer.found_inf
            scaler.update()
        optimizer.zero_grad()
        if ema and getattr(config, 'use_ema_model', False):
            config.ema_model.update(model, skip_flag)

    capture = (graph_inputs is not None and getattr(config, 'use_step_graph', False) and acc_steps == 1
               and _device_of(model).type == 'cuda')

    def whole_step(*tensors):
        packed, _ = forward_backward(tensors, True)
        update(packed)
        return packed

    def graph_for(extra):
        """the step graph of (model, optimizer, *extra), from the cache on the config or new"""
        nonlocal names
        from .. import engine
        cache = getattr(config, '_saicv_step_graphs', None)
        if cache is None:
            cache = {}
            config._saicv_step_graphs = cache       # config is usually a class: the graph lives across epochs
        key = (id(model), id(optimizer)) + extra
        step_graph = cache.get(key)
        if step_graph is None:
            step_graph = engine.StepGraph(whole_step, warmup=getattr(config, 'step_graph_warmup', 3),
                                          before_replay=(optimizer.refresh_hyper,))
            step_graph.loss_term_names = names      # the captured closure writes into THIS list
            cache[key] = step_graph
        else:
            names = step_graph.loss_term_names
        return step_graph

    micro = 0      # accumulation phase counts micro-batches as they are issued; the lagged skip correction in drain() only
                   # moves the logged / scheduled iteration index, never the phase of a window already under way
    for data in train_loader:
        micro += 1
        boundary = micro % acc_steps == 0
        if before_step is not None:
            before_step()
        tensors = graph_inputs(data) if capture else None                    # None: this batch does not fit the captured shapes
        if capture and getattr(graph_inputs, 'may_decline', False) and not all_ranks_agree(tensors is not None, config):
            tensors = None                                                   # ... on SOME rank: every rank takes the eager step
        if tensors is not None:
            step_graph = graph_for(tuple(x for x in tensors if not torch.is_tensor(x)))
            packed = step_graph(*tensors).clone()       # the static output is overwritten by the next replay
            n = tensors[0].size(0)
        else:
            packed, n = forward_backward(data, boundary)
        if carried_bad is not None:
            packed = torch.cat([torch.maximum(packed[0:1], carried_bad), packed[1:]])
        carried_bad = None if boundary else packed[0:1]
        if boundary:
            if tensors is None:
                update(packed)
            scheduler.step(optimizer, iter_index / iters + (epoch - 1))
            log_fmt = None
            if iter_index % int(config.print_interval * acc_steps) == 0:
                log_fmt = (f'train: epoch {epoch:0>4d}, iter [{int(iter_index // acc_steps):0>{iter_width}d}, '
                           f'{int(iters // acc_steps):0>{iter_width}d}], lr: {scheduler.current_lr:.6f}, ' +
                           total_name + (': {loss:.4f}, ' if log_terms else ': {loss:.4f}'))
            pending.append((packed, n, log_fmt))
        drain(lag)
        iter_index += 1
    drain(0)
    return losses.avg * acc_steps


def timed_eval_pass(test_loader, model, config, batch_fn, ema=True):
    """One no-grad pass over `test_loader` with the model in eval() -- the EMA model under config.use_ema_model, unless the caller
    made that switch itself (`ema=False`).  `batch_fn(model, data, device)` is a generator with two `yield`s: the first once the
    batch's inputs are on the device, the second once the forward is issued; what follows (loss, metrics) is untimed.
    -> (load, inference) milliseconds per image of a rank's batch."""
    batch_time, data_time = AverageMeter(), AverageMeter()
    if ema and getattr(config, 'use_ema_model', False):
        model = config.ema_model.ema_model
    model.eval()
    device = _device_of(model)
    sync = torch.cuda.synchronize if device.type == 'cuda' else (lambda: None)
    with torch.no_grad():
        end = time.time()
        for data in test_loader:
            batch = batch_fn(model, data, device)
            next(batch)
            sync()
            data_time.update(time.time() - end)
            end = time.time()
            next(batch)
            sync()
            batch_time.update(time.time() - end)
            for _ in batch:
                pass
            end = time.time()
    per_gpu = config.batch_size // config.gpus_num
    return data_time.avg / per_gpu * 1000, batch_time.avg / per_gpu * 1000


def for_all_datasets(per_dataset_fn):
    """`per_dataset_fn(loader, model, criterion, config)` -> the same over config.val_dataset_name_list / a list of loaders, one result
    per dataset under the reference's key (the dataset's name parts joined by '[+]', '/' written '[s]')"""
    def for_all_dataset(val_loader_list, model, criterion, config):
        result_dict = collections.OrderedDict()
        for name, loader in zip(config.val_dataset_name_list, val_loader_list):
            result_dict['[+]'.join(name).replace('/', '[s]')] = per_dataset_fn(loader, model, criterion, config)
        return result_dict
    return for_all_dataset
