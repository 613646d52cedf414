"""MI355X-native W4A8 static-quant kernels behind MQuant's ``fake_quant`` operator API.

``mquant_amd.ops``   torch-tensor front-end of the C ABI (``include/mquant_hip.h``)
``mquant_amd.kv_cache``  ``Fp8KVCache`` / ``KVCache16``: the e4m3 / 16-bit cache of a captured generation step (its length lives on the device);
                         ``Fp8KVCacheBatch`` / ``KVCache16Batch``: the same for B sequences that step together (B lengths on the device)
``mquant_amd.generate``  ``GreedyLoop``: embed -> layers -> norm -> lm_head -> token as one graph that feeds itself (the token lives there too);
                         ``GreedyLoopBatch``: the same step for B <= 8 sequences per weight pass
``mquant_amd._lib``  ctypes loader of ``libmquant_hip.so`` (no CPU fallback)
``mquant_amd.csrc``  the hand-written gfx950 kernels
"""
__version__ = "0.1.0"


def __getattr__(name):      # the classes of a captured generation step, imported on first use (they pull in torch)
    if name in ("Fp8KVCache", "KVCache16", "Fp8KVCacheBatch", "KVCache16Batch"):
        from . import kv_cache
        return getattr(kv_cache, name)
    if name in ("GreedyLoop", "GreedyLoopBatch"):
        from . import generate
        return getattr(generate, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
