from .device_controller import DeviceController  # noqa: F401
