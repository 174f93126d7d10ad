"""The package's exception, in a module of its own: the host-only data package raises it from loader workers, which must not load
the HIP library (vipant_amd._ffi re-exports it)."""


class VipantError(RuntimeError):
    pass
