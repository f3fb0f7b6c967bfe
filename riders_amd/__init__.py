def freeze_batch_norm(target, freeze=True, affine=True):
    """Freeze (freeze=False: thaw) every BatchNorm2d below an nn.Module, an RCNetModel or an iterable of modules; see engine.freeze_batch_norm."""
    from . import engine
    return engine.freeze_batch_norm(target, freeze, affine)
