"""The reference's `sync_batchnorm` import path over ops.SyncBatchNorm2d, so that a training script changes one import:

    from omnifusion_amd.sync_batchnorm import convert_model
    network = convert_model(network)            # train_erp_depth.py:140; every ops.BatchNorm2d now takes its statistics over all ranks

One process per GPU (omnifusion_amd.dist.init() under the launcher) replaces nn.DataParallel's threads; dist.sync_gradients(network)
before optimizer.step() replaces the gradient reduction of its backward.  The layers of a model's `SYNCBN_REPLICATED` prefixes — those
fed the same input on every rank, whose local statistics ARE the group's — stay unsynchronised.
"""
from .. import ops

SynchronizedBatchNorm2d = ops.SyncBatchNorm2d


def convert_model(module, process_group=None, skip=None):
    """ops.convert_sync_batchnorm on `module`, in place; `skip=None` takes the module's own `SYNCBN_REPLICATED` (a model names the layers
    whose input is identical on every rank).  A 'module.'-prefixed wrapper is not unwrapped: convert the model itself.  Returns the module,
    as the reference's convert_model does."""
    if skip is None:
        skip = getattr(module, "SYNCBN_REPLICATED", ())
    module, _ = ops.convert_sync_batchnorm(module, process_group=process_group, skip=skip)
    return module


class DataParallelWithCallback:
    """Not built: nn.DataParallel runs one thread per GPU inside one process; here one PROCESS per GPU runs the model and the ranks exchange
    statistics (ops.sync_batch_norm) and gradients (dist.sync_gradients)."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("DataParallelWithCallback is not built: start one process per GPU (python -m torch.distributed.run, "
                                  "omnifusion_amd.dist.init()), convert_model(network) and call omnifusion_amd.dist.sync_gradients(network) "
                                  "before optimizer.step() instead of wrapping the model")


__all__ = ["SynchronizedBatchNorm2d", "convert_model", "DataParallelWithCallback"]
