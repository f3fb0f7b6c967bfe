def freeze_batch_norm(target, freeze=True, affine=True):
    """Freeze (freeze=False: thaw) every BatchNorm2d below an nn.Module, an RCNetModel or an iterable of modules; see engine.freeze_batch_norm."""
    from . import engine
    return engine.freeze_batch_norm(target, freeze, affine)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_'s signature: on the device inside a FlatAdam's next step when it can be, torch's own otherwise; see
    optim.clip_grad_norm_."""
    from . import optim
    return optim.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)


def __getattr__(name):
    """`from riders_amd import UTV_dataset`: the reference's class name (data/UTV_dataset.py), bound on first use -- importing the package
    itself stays free of numpy, torch and the HIP library."""
    if name == "UTV_dataset":
        from .utv_dataset import UTV_dataset
        return UTV_dataset
    raise AttributeError("module 'riders_amd' has no attribute %r" % (name,))
