"""The ctypes declarations of libtdec.so (_native._declare) and of libmodem.so
(_native._declare_modem): every export's argument and return types against a literal table,
written out from the assignments each consisted of before it became one table, and not from the
code under test."""
import ctypes as C

from modulations_amd import _native

TYPES = {"int": C.c_int, "long": C.c_long, "double": C.c_double, "float": C.c_float, "void*": C.c_void_p,
         "int64": C.c_int64, "uint64": C.c_uint64, "size_t": C.c_size_t, "uint32": C.c_uint32,
         "longlong": C.c_longlong, "ulonglong": C.c_ulonglong, "char*": C.c_char_p, "void": None,
         "void**": C.POINTER(C.c_void_p), "int*": C.POINTER(C.c_int), "long*": C.POINTER(C.c_long),
         "size_t*": C.POINTER(C.c_size_t), "longlong*": C.POINTER(C.c_longlong)}

# name: (restype, argtypes)
DECLARED = {
    "tdec_create": ("int", "int int int void* int int void* void* void* void**"),
    "tdec_destroy": ("void", "void*"),
    "tdec_last_error": ("char*", ""),
    "tdec_llr_len": ("long", "void*"),
    "tdec_siso_batch": ("int", "void* int void* void* void* void* void* void* double void* void*"),
    "tdec_decode_batch": ("int", "void* int void* long void* void*"),
    "tdec_reserve": ("int", "void* int"),
    "tdec_planes_bytes": ("size_t", "void* int"),
    "tdec_depuncture_dev": ("int", "void* int void* long void* void*"),
    "tdec_decode_planes_dev": ("int", "void* int void* void* void* void*"),
    "tdec_decode_batch_dev": ("int", "void* int void* long void* void* void*"),
    "tdec_tail_gate": ("int", "void* void*"),
    "tdec_demap_dev": ("int", "int void* int long void* int int int double int int void* void*"),
    "tdec_demap": ("int", "int void* int long void* int int int double int int void*"),
    "tdec_demap_planes_dev": ("int", "void* int void* int void* int int int double int void* void*"),
    "tdec_encode_dev": ("int", "void* int void* void* void*"),
    "tdec_encoded_len": ("long", "void*"),
    "tdec_demap_batch": ("int", "int int int void* long float void*"),
    "tdec_constellation": ("int", "int void* int*"),
    "tdec_workload_dev": ("int", "void* int int64 uint64 void* int int double void* void* void*"),
    "tdec_info_bits_dev": ("int", "void* int int64 uint64 void* void*"),
    "tdec_count_errors_dev": ("int", "void* int int64 uint64 void* void* void*"),
    "tdec_reserve_fused": ("int", "void* int"),
    "tdec_fused_available": ("int", "void* int int"),
    "tdec_demap_decode_dev": ("int", "void* int void* int void* int int int double int void* void* void*"),
    "tdec_selftest": ("int", "int int longlong ulonglong longlong*"),
    "tdec_selftest_trans": ("int", "int int uint32 longlong void*"),
    "tdec_host_alloc": ("int", "size_t void**"),
    "tdec_host_free": ("void", "void*"),
    "tdec_encode_host": ("long", "int int void* void* long void* long void* long"),
    "tdec_siso_batch_f64": ("int", "void* int void* void* void* void* void* void* double void* void*"),
    "tdec_siso_staging": ("int", "void* int void** size_t*"),
    "tdec_siso_staged": ("int", "void* int int double"),
    "tdec_siso_stats": ("int", "void* long*"),
    "tdec_decode_batch_es": ("int", "void* int void* long void* void* void*"),
    "tdec_decode_planes_es_dev": ("int", "void* int void* void* void* void* void*"),
    "tdec_decode_batch_es_dev": ("int", "void* int void* long void* void* void* void*"),
    "tdec_es_capacity": ("int", "void*"),
    "tdec_early_stop_available": ("int", "int"),
    "tdec_decode_batch_es_tile": ("int", "void* int void* long void* void* void*"),
    "tdec_decode_planes_es_tile_dev": ("int", "void* int void* void* void* void* void*"),
    "tdec_decode_batch_es_tile_dev": ("int", "void* int void* long void* void* void* void*"),
    "tdec_reserve_es_refill": ("int", "void* int"),
    "tdec_decode_batch_es_refill": ("int", "void* int void* long void* void* void*"),
    "tdec_decode_planes_es_refill_dev": ("int", "void* int void* void* void* void* void*"),
    "tdec_decode_batch_es_refill_dev": ("int", "void* int void* long void* void* void* void*"),
    "tdec_es_refill_stats": ("int", "void* long* long*"),
    "tdec_demap_logmap_dev": ("int", "int void* int long void* int int int double int void* void*"),
    "tdec_demap_logmap": ("int", "int void* int long void* int int int double int void*"),
    "tdec_demap_planes_logmap_dev": ("int", "void* int void* int void* int int int double void* void*"),
    "tdec_noise_var_dev": ("int", "int void* int int void* int int double void* void*"),
    "tdec_demap_rows_dev": ("int", "int void* int int int void* int int int void* int int void* void*"),
    "tdec_demap_rows_logmap_dev": ("int", "int void* int int int void* int int int void* int void* void*"),
    "tdec_demap_planes_nv_dev": ("int", "void* int void* int void* int int int void* int void* void*"),
    "tdec_demap_planes_logmap_nv_dev": ("int", "void* int void* int void* int int int void* void* void*"),
    "tdec_symnv_demap_dev": ("int", "int void* int int int void* int int int void* int int void* void*"),
    "tdec_symnv_demap_logmap_dev": ("int", "int void* int int int void* int int int void* int void* void*"),
    "tdec_symnv_demap_planes_dev": ("int", "void* int void* int void* int int int void* int void* void*"),
    "tdec_symnv_demap_planes_logmap_dev": ("int", "void* int void* int void* int int int void* void* void*"),
    "tdec_equalize_dev": ("int", "int void* void* int int int double void* void* void* void*"),
    "tdec_workload_fading_dev": ("int", "void* int int64 uint64 void* int int double double int void* void* void* void*"),
    "tdec_csi_pilots_dev": ("int", "int void* int int int int void* int double void* double void* void* void* void* "
                                   "void*"),
    "tdec_csi_strip_dev": ("int", "int void* int int int int void* int double void* void* void* void*"),
    "tdec_workload_frame_dev": ("int", "int void* void* int int int int int void* double int64 uint64 double void* "
                                       "void* void*"),
    "tdec_combine_dev": ("int", "int void* void* int int int int double void* void* void* void* void*"),
    "tdec_workload_branches_dev": ("int", "void* int int int64 uint64 void* int int double double int void* void* "
                                          "void* void*"),
    "tdec_workload_frame_branches_dev": ("int", "int void* void* int int int int int int void* double int64 uint64 "
                                                "double void* void* void*"),
}


# libmodem.so (_native._declare_modem), dumped from the one assignment per export it consisted of before
DECLARED_MODEM = {
    "mdm_map_dev": ("int", "int void* long int void* int void* void*"),
    "mdm_map": ("int", "int void* long int void* int void*"),
    "mdm_demod_dev": ("int", "int int void* int long int void* double void* int void* void* void*"),
    "mdm_demod": ("int", "int int void* int long int void* double void* int void*"),
    "mdm_fir_dev": ("int", "int void* int long void* int int int long long void* void*"),
    "mdm_fir": ("int", "int void* int long void* int int int long long void*"),
    "mdm_iq_quantize_dev": ("int", "int void* int long void* void* void*"),
    "mdm_iq_quantize": ("int", "int void* int long void*"),
    "mdm_iq_dequantize_dev": ("int", "int void* long void* void*"),
    "mdm_iq_dequantize": ("int", "int void* long void*"),
    "mdm_last_error": ("char*", ""),
    "mdm_mix_dev": ("int", "int void* int long long void* double double void* void*"),
    "mdm_mix": ("int", "int void* int long long void* double double void*"),
    "mdm_burst_find_dev": ("int", "int void* int long void* int long void* void* void* void*"),
    "mdm_burst_find": ("int", "int void* int long void* int long void* void* void*"),
    "mdm_xcorr_peak_dev": ("int", "int void* long void* int void* void* void* void*"),
    "mdm_xcorr_peak": ("int", "int void* long void* int void* void* void*"),
    "mdm_carrier_dev": ("int", "int void* int long void* void* void* void* void* void* void*"),
    "mdm_carrier": ("int", "int void* int long void* void* void* void* void* void*"),
}


def test_every_modem_export_is_declared_as_before():
    L = _native.modem_lib()
    assert sorted(DECLARED_MODEM) == sorted(_native.MODEM_EXPORTS)
    for name in _native.MODEM_EXPORTS:
        f = getattr(L, name)
        res, args = DECLARED_MODEM[name]
        assert f.restype is TYPES[res], name
        assert list(f.argtypes) == [TYPES[t] for t in args.split()], name


def test_every_export_is_declared_as_before():
    L = _native.lib()
    assert sorted(DECLARED) == sorted(_native.EXPORTS)
    for name in _native.EXPORTS:
        assert hasattr(L, name), name
        f = getattr(L, name)
        res, args = DECLARED[name]
        assert f.restype is TYPES[res], name
        assert list(f.argtypes) == [TYPES[t] for t in args.split()], name

    # the A/B tools load older builds through _declare: what such a build lacks stays undeclared
    class Old:
        tdec_create = type("F", (), {})()
    _native._declare(Old)
    assert Old.tdec_create.restype is C.c_int and len(Old.tdec_create.argtypes) == 10
    assert not hasattr(Old, "tdec_combine_dev")
