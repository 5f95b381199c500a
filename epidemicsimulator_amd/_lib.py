"""ctypes binding of libesim.so (C ABI: include/esim.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C epidemicsimulator_amd/csrc``.
There is no Python or CPU fallback: if the shared object is missing, or no HIP device is
usable, the calls fail loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ESIM_LIB") or os.path.join(_HERE, "libesim.so")   # ESIM_LIB: a diagnostics build of the same library

OK = 0
ERRORS = {-1: "EINVAL", -2: "ENODEVICE", -3: "ENOMEM", -4: "ESTATE", -5: "ERANGE", -6: "ESIM", -7: "ETIMEDOUT"}

SUSCEPTIBLE, EXPOSED, INFECTED, RECOVERED, VACCINATED = range(5)
HOUSEHOLD, WORKPLACE, SCHOOL = range(3)
MASK_NONE, MASK_PUBLIC_TRANSPORT, MASK_EVERYWHERE = range(3)
NO_ROOM = 0xFFFFFFFF
FLAG_USES_PUBLIC_TRANSPORT = 1
FLAG_MASK_COMPLIANT = 2


class EsimError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libesim %s (%d): %s" % (ERRORS.get(code, "?"), code, text))
        self.code = code


class Params(C.Structure):
    _fields_ = [
        ("exposure_chance", C.c_double), ("mask_effectiveness", C.c_double),
        ("lockdown_threshold", C.c_double), ("vaccination_threshold", C.c_double),
        ("mask_pt_threshold", C.c_double), ("mask_everywhere_threshold", C.c_double),
        ("exposed_time", C.c_uint32), ("infected_time", C.c_uint32),
        ("vaccination_rate", C.c_uint32), ("bus_capacity", C.c_uint32),
        ("start_hour", C.c_uint32), ("end_hour", C.c_uint32),
        ("seed", C.c_uint64), ("device", C.c_int32), ("max_steps", C.c_uint32),
    ]


_u32p, _u16p, _u8p, _i32p = (C.POINTER(C.c_uint32), C.POINTER(C.c_uint16),
                             C.POINTER(C.c_uint8), C.POINTER(C.c_int32))


class PopulationStruct(C.Structure):
    _fields_ = [
        ("n_citizens", C.c_uint32), ("n_buildings", C.c_uint32), ("n_areas", C.c_uint32),
        ("n_rooms", C.c_uint32), ("n_seeds", C.c_uint32),
        ("citizen_id_base", C.c_uint32), ("n_citizens_global", C.c_uint32),
        ("n_shared_buildings", C.c_uint32), ("n_shared_rooms", C.c_uint32),
        ("home_building", _u32p), ("work_building", _u32p), ("room", _u32p),
        ("flags", _u8p), ("age", _u16p), ("occupation", _u8p),
        ("building_area", _u32p), ("building_type", _u8p), ("room_building", _u32p),
        ("seeds", _u32p), ("shared_building_local", _i32p), ("shared_room_local", _i32p),
    ]


class StepResult(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "time_step", "susceptible", "exposed", "infected", "recovered", "vaccinated",
        "exposures_building", "exposures_bus", "lockdown", "vaccination_active", "mask_status",
        "n_riders", "vaccinated_now", "eligible_count", "disease_exists", "reserved")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


RECORD_FIELDS = [n for n, _ in StepResult._fields_]


class BurdenParams(C.Structure):
    _fields_ = [
        ("n_groups", C.c_uint32), ("admit_thr", _u32p), ("death_thr", _u32p),
        ("delay_unit", C.c_uint32), ("n_delay", C.c_uint32), ("delay_cdf", _u32p),
        ("stay_unit", C.c_uint32), ("n_stay", C.c_uint32), ("stay_cdf", _u32p),
    ]


class SynthSpec(C.Structure):
    _fields_ = [
        ("n_citizens", C.c_uint32), ("n_areas", C.c_uint32), ("citizens_per_school", C.c_uint32),
        ("n_seeds", C.c_uint32), ("seed", C.c_uint64), ("area_jitter", C.c_double),
        ("p_public_transport", C.c_double), ("p_mask_compliant", C.c_double),
        ("p_work_from_home", C.c_double), ("p_teaching", C.c_double),
        ("household_buildings_median", C.c_double), ("household_buildings_sigma", C.c_double),
        ("p_area_without_households", C.c_double),
        ("workplace_buildings_median", C.c_double), ("workplace_buildings_sigma", C.c_double),
        ("p_area_without_workplaces", C.c_double),
        ("workplace_floor_median", C.c_double), ("workplace_floor_sigma", C.c_double),
        ("teacher_candidate_schools", C.c_uint32), ("reserved", C.c_uint32),
    ]


# every symbol include/esim.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = [
    "esim_default_params", "esim_create", "esim_upload_population", "esim_reset", "esim_restart", "esim_restart_seeded", "esim_get_seeds", "esim_step",
    "esim_run", "esim_set_pipeline", "esim_chunk_timing", "esim_enable_chunk_kernel_timing", "esim_chunk_kernel_timings", "esim_vax_chunk_stats", "esim_vax_repair_stats", "esim_pipeline_timing",
    "esim_comm_unique_id", "esim_comm_init_rccl", "esim_comm_init_callback", "esim_comm_set_timeout", "esim_debug_inject_error", "esim_comm_stats", "esim_run_sharded", "esim_shard_stats",
    "esim_read_records", "esim_synchronize",
    "esim_download_state", "esim_download_exposure_log", "esim_area_census", "esim_area_arrival", "esim_area_series", "esim_area_status_series", "esim_set_groups", "esim_group_census", "esim_group_series", "esim_exposure_settings", "esim_setting_series", "esim_building_exposures", "esim_transmission_tree", "esim_offspring", "esim_reproduction_series", "esim_mixing_matrix", "esim_transmission_chains", "esim_outbreaks", "esim_transmission_ages", "esim_household_outbreaks", "esim_household_final_sizes", "esim_household_sar", "esim_place_outbreaks", "esim_place_sizes", "esim_place_sar", "esim_contact_hours", "esim_area_flows", "esim_area_imports", "esim_area_invasion", "esim_lineage_areas", "esim_pair_stats", "esim_transmission_events", "esim_routes", "esim_ensemble_begin", "esim_ensemble_begin_arrival", "esim_ensemble_fold", "esim_ensemble_read", "esim_ensemble_begin_series", "esim_ensemble_read_series", "esim_ensemble_begin_settings", "esim_ensemble_begin_reproduction", "esim_ensemble_read_reproduction", "esim_checkpoint_size", "esim_checkpoint_save", "esim_checkpoint_restore", "esim_snapshot", "esim_rollback", "esim_snapshot_info", "esim_snapshot_drop", "esim_baseline_keep", "esim_baseline_info", "esim_baseline_drop", "esim_compare", "esim_compare_series", "esim_ensemble_begin_paired", "esim_ensemble_read_paired", "esim_curve_summary", "esim_ensemble_begin_peaks", "esim_ensemble_read_peaks",
    "esim_burden_set", "esim_burden_drop", "esim_burden_get", "esim_burden_outcomes", "esim_burden_series", "esim_burden_summary", "esim_ensemble_begin_burden_peaks",
    "esim_burden_baseline_keep", "esim_burden_baseline_info", "esim_burden_baseline_drop", "esim_burden_baseline_read", "esim_burden_compare", "esim_burden_compare_series",
    "esim_ensemble_begin_burden_series", "esim_ensemble_begin_burden_paired",
    "esim_ensemble_keep_members", "esim_ensemble_members_info", "esim_ensemble_read_members", "esim_ensemble_quantiles", "esim_ensemble_exceedance", "esim_ensemble_depth", "esim_ensemble_band", "esim_ensemble_distances", "esim_ensemble_distances_info", "esim_ensemble_arms", "esim_ensemble_merge", "esim_ensemble_save_size", "esim_ensemble_save", "esim_ensemble_load", "esim_enable_phase_timing", "esim_phase_timings",
    "esim_enable_kernel_timing", "esim_kernel_timings", "esim_set_small_step_limit", "esim_set_tiny_chunk_limit", "esim_small_kernel_timing", "esim_debug_counters", "esim_debug_launches",
    "esim_last_error", "esim_destroy",
    "esim_threshold_lut", "esim_synth_preset", "esim_synth_create", "esim_synth_create_shard", "esim_synth_free",
    "esim_shard_population", "esim_shard_cuts",
]

# esim_allreduce_fn: int (*)(void *user, int which, void *device_ptr, size_t n_u32)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t)

_lib = None


def load():
    """Loads libesim.so (once).  Raises if it has not been built -- no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libesim.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C epidemicsimulator_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    sig = {
        "esim_default_params": (None, [C.POINTER(Params)]),
        "esim_create": (C.c_int, [C.POINTER(Params), pvp]),
        "esim_upload_population": (C.c_int, [vp, C.POINTER(PopulationStruct)]),
        "esim_reset": (C.c_int, [vp]),
        "esim_restart": (C.c_int, [vp, C.POINTER(Params)]),
        "esim_restart_seeded": (C.c_int, [vp, C.POINTER(Params), _u32p, C.c_uint32]),
        "esim_get_seeds": (C.c_int, [vp, _u32p, C.c_uint32, _u32p]),
        "esim_step": (C.c_int, [vp, C.POINTER(StepResult)]),
        "esim_run": (C.c_int, [vp, C.c_uint32, C.c_int, C.POINTER(StepResult), C.POINTER(C.c_uint32)]),
        "esim_comm_unique_id": (C.c_int, [vp, C.c_size_t]),
        "esim_comm_init_rccl": (C.c_int, [vp, vp, C.c_size_t, C.c_int, C.c_int]),
        "esim_comm_init_callback": (C.c_int, [vp, ALLREDUCE_FN, vp, C.c_int, C.c_int]),
        "esim_comm_set_timeout": (C.c_int, [vp, C.c_double]),
        "esim_debug_inject_error": (C.c_int, [vp, C.c_int]),
        "esim_comm_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "esim_run_sharded": (C.c_int, [vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "esim_shard_stats": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_set_pipeline": (C.c_int, [vp, C.c_int]),
        "esim_chunk_timing": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_enable_chunk_kernel_timing": (C.c_int, [vp, C.c_int]),
        "esim_chunk_kernel_timings": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "esim_vax_chunk_stats": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_vax_repair_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "esim_pipeline_timing": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_read_records": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.POINTER(StepResult)]),
        "esim_synchronize": (C.c_int, [vp]),
        "esim_download_state": (C.c_int, [vp, _u8p, _u16p, _u32p, _u8p, _u8p]),
        "esim_download_exposure_log": (C.c_int, [vp, _u32p, _u32p, _u8p, C.c_uint32, _u32p]),
        "esim_area_census": (C.c_int, [vp, C.c_int, _u32p]),
        "esim_area_arrival": (C.c_int, [vp, C.c_int, _u32p]),
        "esim_area_series": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
        "esim_area_status_series": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
        "esim_set_groups": (C.c_int, [vp, _u16p, C.c_uint32]),
        "esim_group_census": (C.c_int, [vp, _u32p]),
        "esim_group_series": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
        "esim_exposure_settings": (C.c_int, [vp, _u8p, _u32p]),
        "esim_setting_series": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
        "esim_building_exposures": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p]),
        "esim_transmission_tree": (C.c_int, [vp, _u32p, _u32p, _u32p]),
        "esim_offspring": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p]),
        "esim_reproduction_series": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p]),
        "esim_mixing_matrix": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
        "esim_transmission_chains": (C.c_int, [vp, _u32p, _u32p]),
        "esim_outbreaks": (C.c_int, [vp, _u32p, _u32p, _u32p, C.c_uint32, _u32p]),
        "esim_transmission_ages": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p]),
        "esim_household_outbreaks": (C.c_int, [vp, _u32p, _u32p, _u32p]),
        "esim_household_final_sizes": (C.c_int, [vp, _u32p, _u32p]),
        "esim_household_sar": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_place_outbreaks": (C.c_int, [vp, C.c_int, _u32p, _u32p, _u32p, _u32p]),
        "esim_place_sizes": (C.c_int, [vp, C.c_int, _u32p, _u32p]),
        "esim_place_sar": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_contact_hours": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _u32p]),
        "esim_area_flows": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p, C.c_uint32, _u32p]),
        "esim_area_imports": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p]),
        "esim_area_invasion": (C.c_int, [vp, _u32p, _u32p, _u32p, _u8p]),
        "esim_lineage_areas": (C.c_int, [vp, _u32p, _u32p, _u32p, C.c_uint32, _u32p]),
        "esim_pair_stats": (C.c_int, [vp, C.POINTER(C.c_double), _u32p]),
        "esim_transmission_events": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u32p, _u8p, _u32p, _u32p, _u32p, C.c_uint32, _u32p, _u32p]),
        "esim_routes": (C.c_int, [vp, _u32p, _u32p, _u32p, C.c_uint32, _u32p]),
        "esim_ensemble_begin": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32]),
        "esim_ensemble_begin_arrival": (C.c_int, [vp, C.c_int, C.c_uint32]),
        "esim_ensemble_fold": (C.c_int, [vp]),
        "esim_ensemble_read": (C.c_int, [vp, _u32p, _u32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_ensemble_begin_series": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "esim_ensemble_read_series": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, _u32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_ensemble_begin_settings": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "esim_ensemble_begin_reproduction": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "esim_ensemble_read_reproduction": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p] + [C.POINTER(C.c_uint64)] * 5),
        "esim_checkpoint_size": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
        "esim_checkpoint_save": (C.c_int, [vp, vp, C.c_size_t]),
        "esim_checkpoint_restore": (C.c_int, [vp, vp, C.c_size_t]),
        "esim_snapshot": (C.c_int, [vp]),
        "esim_rollback": (C.c_int, [vp, C.POINTER(Params)]),
        "esim_snapshot_info": (C.c_int, [vp, _u32p, C.POINTER(Params)]),
        "esim_snapshot_drop": (C.c_int, [vp]),
        "esim_baseline_keep": (C.c_int, [vp]),
        "esim_baseline_info": (C.c_int, [vp, _u32p, _u32p, C.POINTER(Params)]),
        "esim_baseline_drop": (C.c_int, [vp]),
        "esim_compare": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), _u32p, _u8p]),
        "esim_compare_series": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u32p, _u32p]),
        "esim_ensemble_begin_paired": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32]),
        "esim_ensemble_read_paired": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p] + [C.POINTER(C.c_uint64)] * 5),
        "esim_curve_summary": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _u32p, C.POINTER(C.c_uint64)]),
        "esim_ensemble_begin_peaks": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "esim_ensemble_read_peaks": (C.c_int, [vp, _u32p, _u32p, _u32p] + [C.POINTER(C.c_uint64)] * 6),
        "esim_burden_set": (C.c_int, [vp, C.POINTER(BurdenParams)]),
        "esim_burden_drop": (C.c_int, [vp]),
        "esim_burden_get": (C.c_int, [vp] + [_u32p] * 9),
        "esim_burden_outcomes": (C.c_int, [vp, _u32p, _u32p, _u8p]),
        "esim_burden_series": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
        "esim_burden_summary": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _u32p, C.POINTER(C.c_uint64), _u32p, _u32p]),
        "esim_ensemble_begin_burden_peaks": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "esim_burden_baseline_keep": (C.c_int, [vp]),
        "esim_burden_baseline_info": (C.c_int, [vp, _u32p, _u32p, _u32p, C.POINTER(Params)]),
        "esim_burden_baseline_drop": (C.c_int, [vp]),
        "esim_burden_baseline_read": (C.c_int, [vp, _u32p, _u32p, _u32p, _u8p, C.c_uint32, _u32p]),
        "esim_burden_compare": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _u32p, _u32p, _u32p, _u32p]),
        "esim_burden_compare_series": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u32p, _u32p]),
        "esim_ensemble_begin_burden_series": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "esim_ensemble_begin_burden_paired": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32]),
        "esim_ensemble_keep_members": (C.c_int, [vp, C.c_uint32, C.c_int]),
        "esim_ensemble_members_info": (C.c_int, [vp, _u32p, _u32p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "esim_ensemble_read_members": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
        "esim_ensemble_quantiles": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _u32p]),
        "esim_ensemble_exceedance": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64), C.c_uint32, _u32p]),
        "esim_ensemble_depth": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, C.POINTER(C.c_uint64)]),
        "esim_ensemble_band": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u32p, _u32p, _u32p, _u32p, _u32p]),
        "esim_ensemble_distances": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_ensemble_distances_info": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_ensemble_arms": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "esim_ensemble_merge": (C.c_int, [vp, vp]),
        "esim_ensemble_save_size": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
        "esim_ensemble_save": (C.c_int, [vp, vp, C.c_size_t]),
        "esim_ensemble_load": (C.c_int, [vp, vp, C.c_size_t]),
        "esim_enable_phase_timing": (C.c_int, [vp, C.c_int]),
        "esim_phase_timings": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "esim_enable_kernel_timing": (C.c_int, [vp, C.c_int]),
        "esim_kernel_timings": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
        "esim_debug_counters": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "esim_debug_launches": (C.c_int, [vp, C.c_char_p, _u32p, C.c_uint32, _u32p, C.c_int]),
        "esim_set_small_step_limit": (C.c_int, [vp, C.c_uint32]),
        "esim_set_tiny_chunk_limit": (C.c_int, [vp, C.c_uint32]),
        "esim_small_kernel_timing": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "esim_last_error": (C.c_char_p, [vp]),
        "esim_destroy": (None, [vp]),
        "esim_threshold_lut": (C.c_int, [C.POINTER(Params), C.POINTER(C.c_uint64)]),
        "esim_synth_preset": (C.c_int, [C.c_char_p, C.POINTER(SynthSpec)]),
        "esim_synth_create": (C.c_int, [C.POINTER(SynthSpec), C.POINTER(PopulationStruct)]),
        "esim_synth_create_shard": (C.c_int, [C.POINTER(SynthSpec), C.c_uint32, C.c_uint32, C.POINTER(PopulationStruct)]),
        "esim_shard_cuts": (C.c_int, [C.POINTER(PopulationStruct), C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
        "esim_synth_free": (None, [C.POINTER(PopulationStruct)]),
        "esim_shard_population": (C.c_int, [C.POINTER(PopulationStruct), _u32p, C.c_uint32, C.c_uint32,
                                            C.POINTER(PopulationStruct)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


ESIM_OK, ESIM_ERANGE = 0, -5          # include/esim.h
AREA_CURRENT, AREA_HOME = 0, 1        # esim_area_census `where`
SERIES_INFECTED, SERIES_EXPOSURES = 0, 1   # esim_area_series `what`
BY_GROUP = 2                          # esim_ensemble_begin `where`, beside AREA_CURRENT and AREA_HOME
MAX_GROUPS = 1024                     # ESIM_MAX_GROUPS
NEVER = 0xFFFFFFFF                    # ESIM_NEVER: esim_area_arrival's entry for an area or group not reached
GROUP_SERIES_EXPOSURES = 5            # esim_group_series `what`, beside the five status codes
AREA_SERIES_INCIDENCE = 5             # esim_area_status_series `what`, beside the five status codes
SETTING_HOUSEHOLD, SETTING_WORKPLACE, SETTING_SCHOOL, SETTING_TRANSPORT = range(4)   # ESIM_SETTING_*
N_SETTINGS = 4
SETTING_NONE = 0xFF                   # a citizen never exposed, an index case, an unexplained entry
SETTING_NAMES = ("household", "workplace", "school", "transport")
BY_SETTING = 3                        # esim_setting_series `where`, beside AREA_HOME and BY_GROUP
NO_INFECTOR = 0xFFFFFFFF              # ESIM_NO_INFECTOR: esim_transmission_tree's entry for an index case, a citizen never exposed, an unexplained entry
BY_ALL = 4                            # esim_reproduction_series `where`, beside AREA_HOME and BY_GROUP: one column
NO_LINEAGE = 0xFFFFFFFF               # ESIM_NO_LINEAGE: esim_transmission_chains' entry for a citizen whose chain reaches no index case
MEMBERS_MAX, RANKS_MAX = 256, 16      # ESIM_MEMBERS_MAX, ESIM_RANKS_MAX: esim_ensemble_keep_members' capacity, ranks or thresholds a call
KEEP_VALUE, KEEP_PEAK_STEP, KEEP_DURATION = range(3)   # ESIM_KEEP_*: `what` of esim_ensemble_keep_members
DIST_L1, DIST_DIFFER = range(2)       # ESIM_DIST_*: `metric` of esim_ensemble_distances
ARMS_MAX = 16                         # ESIM_ARMS_MAX: the arms of esim_ensemble_arms
BURDEN_BINS = 64                      # ESIM_BURDEN_BINS: the most entries of a delay or stay CDF of esim_burden_set
BURDEN_ADMISSIONS, BURDEN_OCCUPANCY, BURDEN_DEATHS = range(3)   # ESIM_BURDEN_*: `what` of esim_burden_series
BURDEN_NAMES = ("admissions", "occupancy", "deaths")
AGE_BINS = 512                     # ESIM_AGE_BINS: the infectious ages esim_transmission_ages counts per setting
HH_BINS = 64                          # ESIM_HH_BINS: household sizes and case counts of esim_household_final_sizes, the last bin open-ended
PLACE_WORK, PLACE_ROOM, PLACE_SCHOOL = range(3)   # ESIM_PLACE_*: the `kind` of esim_place_outbreaks, esim_place_sizes, esim_place_sar
PLACE_NAMES = ("work", "room", "school")
PLACE_BINS = 32                       # ESIM_PLACE_BINS: sizes and case counts of esim_place_sizes, exact below 16, then a bin per power of two
NO_AREA = 0xFFFFFFFF                  # ESIM_NO_AREA: esim_area_invasion's source_area for an index case, an area without a case, an unexplained entry
EVENT_BINS = 256                      # ESIM_EVENT_BINS: the event sizes esim_transmission_events counts per setting, the last bin open-ended
EVENTS_BY_KEY, EVENTS_BY_SIZE = 0, 1  # esim_transmission_events `order`
CMP_BOTH, CMP_AVERTED, CMP_ADDED, CMP_EARLIER, CMP_LATER = range(5)   # ESIM_CMP_*: the classes of esim_compare
CMP_N = 5
CMP_NAMES = ("both", "averted", "added", "earlier", "later")
ENSEMBLE_SERIES_EVENTS = 5            # esim_ensemble_begin_series `what`, beside the five status codes: incidence / exposures
DEBUG_COUNTERS = ("t", "chunk_ok", "chunk_parallel", "chunk_pairs", "n_items", "items_per_wave", "n_units", "chunk_bus",
                  "n_route_pairs_big", "n_newexp", "log_len", "n_susceptible", "lockdown", "mask", "at_work", "bus_dir")   # esim_debug_counters
LAUNCH_SITE_CHARS = 48                # ESIM_LAUNCH_SITE_CHARS: a site's name in esim_debug_launches
LAUNCH_SITES_MAX = 128                # the sites esim_debug_launches can hold
CHUNK_KERNELS = ("marks", "fold", "draw", "units", "count", "books", "scatter", "vax", "vax_adj", "vax_final", "decide", "future", "map_clear", "tiny", "vax_repair")   # ESIM_CK_* (vax_adj, map_clear: always 0)
PHASE_OF_KERNEL = {"marks": "Generate Exposures", "fold": "Generate Exposures", "draw": "Apply Exposures", "units": "Apply Exposures"}   # the rest: "Apply Interventions"
TINY_PHASE_SHARES = {"Generate Exposures": 0.10, "Apply Exposures": 0.40, "Apply Interventions": 0.50}   # k_chunk_tiny: all three in one launch


def check(code, ctx=None):
    if code != OK:
        text = load().esim_last_error(ctx)
        raise EsimError(code, text.decode() if text else "")


def with_overrides(params, overrides):
    """A copy of `params` with the fields of the dict `overrides` set; AttributeError for a field esim_params does not have."""
    p = Params()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(Params))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError("esim_params has no field %r" % k)
        setattr(p, k, v)
    return p


def default_params(**overrides):
    p = Params()
    load().esim_default_params(C.byref(p))
    return with_overrides(p, overrides)


def _burden_words(who, x):
    """A table as uint32 words: integers as they are, probabilities p as min(int(p * 2**32), 0xFFFFFFFF)."""
    import numpy as np
    a = np.atleast_1d(np.asarray(x))
    if a.ndim != 1:
        raise ValueError("burden_tables: %s must be one-dimensional" % who)
    if a.dtype.kind in "ui":
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("burden_tables: %s holds an integer outside uint32" % who)
        return a.astype(np.uint32)
    if a.size and not ((a >= 0.0) & (a <= 1.0)).all():
        raise ValueError("burden_tables: %s holds a probability outside [0, 1]" % who)
    return np.array([min(int(float(p) * 2 ** 32), 0xFFFFFFFF) for p in a], np.uint32)


def burden_tables(p_admit, p_death, delay_pmf, stay_pmf, delay_unit=24, stay_unit=24):
    """The severity tables of esim_burden_set as a dict of uint32 arrays and the two units.  p_admit, p_death: one entry per
    group, probabilities (thresholds by min(int(p * 2**32), 0xFFFFFFFF)) or integer thresholds, taken as they are.  delay_pmf:
    the probabilities of a delay of 0, 1, 2, ... units between onset and admission; stay_pmf: those of a stay of 1, 2, 3, ...
    units.  Their cumulative sums become the CDFs the same way: n entries give n + 1 outcomes, the last one with the
    probability that is left (a pmf given in full ends in a CDF entry that only the largest draw reaches).  Integer arrays are
    taken as the CDFs themselves."""
    import numpy as np

    def cdf(who, pmf):
        a = np.atleast_1d(np.asarray(pmf))
        return _burden_words(who, a if a.dtype.kind in "ui" else np.minimum(np.cumsum(a.astype(np.float64)), 1.0))

    out = dict(admit_thr=_burden_words("p_admit", p_admit), death_thr=_burden_words("p_death", p_death), delay_cdf=cdf("delay_pmf", delay_pmf),
               stay_cdf=cdf("stay_pmf", stay_pmf), delay_unit=int(delay_unit), stay_unit=int(stay_unit))
    if out["admit_thr"].shape != out["death_thr"].shape:
        raise ValueError("burden_tables: p_admit and p_death must have one entry per group each")
    return out
