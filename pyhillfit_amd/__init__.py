"""pyhillfit_amd — MI355X-native Metropolis-Hastings engine for PyHillFit's sampling step.

Host side in Python on PyTorch-ROCm tensors (device memory, streams, torch.distributed only);
the sampler is hand-written HIP behind the C ABI of include/pyhillfit_amd.h."""
__version__ = "0.1.0"

# The ROCm runtime's hardware-queue count (GPU_MAX_HW_QUEUES) is left to the environment: the hierarchical groups the
# gfx950 code object has kernels for share ONE persistent grid on one stream (every Crumb group does), so only the
# --fused-launch off arrangement, one stream per group, has kernels that could wait for a free queue.
