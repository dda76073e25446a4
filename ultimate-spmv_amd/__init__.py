"""uspmv-mi355x: MI355X-native SELL-C-sigma SpMV / SpMMV engine.

The product is the C-ABI shared library ``libuspmv.so`` (host data layer in C++, hand-written
HIP kernels for gfx950; see include/uspmv.h).  This package is only the thin ctypes front-end used
by tests/, bench.py and __graft_entry__.py, plus the torch.distributed (RCCL) halo-exchange
driver.  It never imports anything from ``oracle/`` and has no CPU fallback: device entry points
raise UspmvError when the HIP extension or a GPU is missing.

The directory name contains a hyphen (repository convention), so import it through
``__graft_entry__.load_package()`` (module name ``ultimate_spmv_amd``).
"""
from .binding import (  # noqa: F401
    AP_DP_HP, AP_DP_SP, AP_DP_SP_HP, AP_SP_HP, COLWISE, F16, F32, F64, ROWWISE, SEG_NNZ, SEG_ROWS, Coo, DeviceMatrix, HaloPlan, Scs, UspmvError, apply_permutation,
    build_library, convert_to_scs, convert_to_scs_device, convert_to_scs_device_from_arrays, convert_ap_device_from_arrays, partition_precisions_device, SORT_HOST, SORT_DEVICE_STABLE, device_count, dmat_download, gen_banded_random, graph_partition, read_partition, apply_partition, gen_kkt, gen_kkt_row_counts, gen_stencil27, get_tuning, lib, library_path, optimize_ap, optimize_ap_hp, optimize_device_ap, optimize_device_ap_hp, optimize_sweep_ap, optimize_sweep_ap_hp, optimize_sweep_device_ap_hp, pack_send_buf,
    partition_precisions, partition_precisions_hp, permute_scs_cols, read_mtx, seg_work_sharing_arr, seg_local_coo, set_tuning, spmmv_x_prepared, spmmv_x_release, spmmv, spmmv_ap, spmmv_ap_path, spmmv_ap_plan_lines, spmmv_ap_sweep_vectors, spmmv_ap_hp, spmmv_ap_hp_path, spmmv_ap_hp_plan_lines, spmmv_ap_hp_sweep_vectors, spmv, spmv_ap, spmv_ap_hp, additive_plan_probe, additive_plan_probe2,
    spmv_chunks, spmv_tiles, spmv_axpby, spmv_axpby_path, AxpbyOp, spmv_ap_axpby, spmv_ap_axpby_path, ap_axpby_reserve, spmv_ap_hp_axpby, spmv_ap_hp_axpby_path, ap_hp_axpby_reserve, uspmv_csr_gpu, uspmv_scs_gpu, DistNative, HostComm, CommPlan, Transport, DistOptions, EXCHANGE_HOST, EXCHANGE_PEER, EXCHANGE_RCCL, runtime_versions, dist_check_reference, comm_unique_id, seg_from_row_counts, gen_stencil27_row_counts,
    halo_discover_device, ONE_PRECISION, gen_stencil27_device,
    raw_plan_cache_values_changed, REFRESH_COPIES, REFRESH_RECHUNKED, REFRESH_SWEEP_REBUILT, REFRESH_BLOCK_SWEEP_DROPPED,
    partition_precisions_eq, equilibrate_device, equilibrate_device_count_atomics, partition_precisions_device_eq, convert_ap_device_from_arrays_eq,
    halo_discover_ap, spmv_ap_tiles, spmv_ap_chunks, spmmv_ap_tiles, spmmv_ap_chunks, spmmv_ap_tiles_path, dist_check_reference_ap,
    halo_discover_ap_hp, spmv_ap_hp_tiles, spmv_ap_hp_chunks, spmmv_ap_hp_tiles, spmmv_ap_hp_chunks, spmmv_ap_hp_tiles_path, dist_check_reference_ap_hp,
)

__version__ = "0.2.0"
