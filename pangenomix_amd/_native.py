"""ctypes binding of libpgx.so (include/pgx.h). Thin on purpose: argument marshalling
and error translation only. There is no CPU fallback -- if the library or a GPU is
missing, the first compute call raises PgxError."""

import ctypes as C
import importlib.util
import os
import threading

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libpgx.so')


class PgxError(RuntimeError):
    pass


class DeviceInfo(C.Structure):
    _fields_ = [('name', C.c_char * 64), ('arch', C.c_char * 32), ('device_id', C.c_int32),
                ('compute_units', C.c_int32), ('wavefront_size', C.c_int32),
                ('lds_bytes_per_block', C.c_int32), ('hbm_bytes', C.c_uint64),
                ('clock_khz', C.c_int32), ('reserved', C.c_int32)]


# int (*exchange)(void *user, void *stream, int slot): enqueue the all-gather of a window's best keys (pgx.h)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
EXCHANGE_KEYS = 65536                  # PGX_EXCHANGE_KEYS
EXCHANGE_WORDS = EXCHANGE_KEYS + 8     # PGX_EXCHANGE_WORDS: the keys + the error word (+ padding)
EXCHANGE_SLOTS = 2                     # PGX_EXCHANGE_SLOTS: windows in flight


class ClusterParams(C.Structure):
    _fields_ = [('alphabet', C.c_int32), ('word_len', C.c_int32), ('band_width', C.c_int32),
                ('min_length', C.c_int32), ('both_strands', C.c_int32), ('batch_size', C.c_int32),
                ('identity', C.c_double), ('aan_cutoff', C.c_double), ('aas_cutoff', C.c_double),
                # record-sharded multi-GPU mode (all zero / NULL = single GPU)
                ('shard_index', C.c_int32), ('shard_count', C.c_int32),
                ('exchange', EXCHANGE_FN), ('exchange_user', C.c_void_p), ('exchange_send', C.c_void_p),
                ('exchange_recv', C.c_void_p),
                # cd-hit's memory-chunked rule: flush positions in the sorted list (NULL = unchunked)
                ('chunk_boundaries', C.POINTER(C.c_uint32)), ('n_chunk_boundaries', C.c_uint32), ('reserved0', C.c_uint32)]


STAT_FIELDS = ('n_input', 'n_clustered', 'n_clusters', 'sum_len_queries', 'sum_len_reps', 'rep_words',
               'posting_visits', 'filter_pairs', 'aligned_pairs', 'aligned_rep_len', 'dp_cells', 'sweeps')


class ClusterStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in STAT_FIELDS] + [('reserved', C.c_uint64 * 4)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n in STAT_FIELDS}
        d['gpu'] = {'pairs': int(self.reserved[0]), 'aligned': int(self.reserved[1]),
                    'aligned_bytes': int(self.reserved[2]), 'filter_walk_words': int(self.reserved[3])}
        return d


class FastaInfo(C.Structure):
    _fields_ = [('n_records', C.c_uint64), ('n_missing', C.c_uint64), ('n_groups', C.c_uint64),
                ('n_residue_bytes', C.c_uint64), ('n_header_bytes', C.c_uint64), ('simple', C.c_uint32),
                ('reserved', C.c_uint32), ('why', C.c_char * 256)]


class FcdInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ('n_concepts', 'n_row_entries', 'n_col_entries', 'steps', 'ones_total',
                                          'ones_left')]


FCD_OVERLAP, FCD_DIM_BALANCE = 1, 2    # PGX_FCD_OVERLAP, PGX_FCD_DIM_BALANCE
BERNOULLI_CD_LOGS = 1                  # PGX_BERNOULLI_CD_LOGS
ASSOC_BLOCKS, ASSOC_DROP_EMPTY = 1, 2  # PGX_ASSOC_BLOCKS, PGX_ASSOC_DROP_EMPTY
DICT_NARROW_HASH = 1                   # PGX_DICT_NARROW_HASH
PATTERN_NARROW_HASH = 1                # PGX_PATTERN_NARROW_HASH
NEAR_NARROW_HASH = 1                   # PGX_NEAR_NARROW_HASH
NEAR_NO_SEPARATOR = 0x100              # PGX_NEAR_NO_SEPARATOR
PROX_NARROW_HASH = 1                 # PGX_PROX_NARROW_HASH
ANNOT_NARROW_HASH = 1                  # PGX_ANNOT_NARROW_HASH
ASSOC_NARROW_HASH = 4                  # PGX_ASSOC_NARROW_HASH
TERM_FOLD_ASCII = 1                    # PGX_TERM_FOLD_ASCII
TERM_MAX_TERMS = 512                   # PGX_TERM_MAX_TERMS
TERM_MAX_BYTES = 32768                 # PGX_TERM_MAX_BYTES
TUPLE_NARROW_HASH = 1                  # PGX_TUPLE_NARROW_HASH
TUPLE_MAX_COLUMNS = 8                  # PGX_TUPLE_MAX_COLUMNS


# every symbol include/pgx.h declares: (restype, argtypes)
_P = C.c_void_p
_S = C.c_char_p
SIGNATURES = {
    'pgx_fasta_open': (C.c_int, [C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.POINTER(_P)]),
    'pgx_fasta_close': (None, [_P]),
    'pgx_fasta_info': (C.c_int, [_P, C.POINTER(FastaInfo)]),
    'pgx_fasta_group_of_record': (_P, [_P]),
    'pgx_fasta_file_of_record': (_P, [_P]),
    'pgx_fasta_rep_of_group': (_P, [_P]),
    'pgx_fasta_residues': (_P, [_P]),
    'pgx_fasta_offsets': (_P, [_P]),
    'pgx_fasta_letters': (_P, [_P]),
    'pgx_fasta_digests': (_P, [_P]),
    'pgx_fasta_header_blob': (_P, [_P]),
    'pgx_fasta_header_offsets': (_P, [_P]),
    'pgx_fasta_write_consolidated': (C.c_int, [_P, _S, _S, _S]),
    'pgx_legacy_shuffles': (C.c_int, [_P, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, _P]),
    'pgx_legacy_uniform_words': (C.c_int, [_P, C.POINTER(C.c_int32), C.c_uint64, _P]),
    'pgx_pan_core_table': (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_int32), C.c_uint32,
                                    _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    'pgx_bitmap_from_clusters': (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_uint64)]),
    'pgx_bitmap_resident_read': (C.c_int, [_P, C.c_uint64, _P]),
    'pgx_pan_core_table_resident': (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_int32), C.c_uint32, _P, _P]),
    'pgx_allele_order': (C.c_int, [_P, _P, C.c_uint64, _P]),
    'pgx_fasta_feature_coo': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _P, _P,
                                       C.POINTER(C.c_uint64), _P, _P, C.POINTER(C.c_uint64), _P, C.POINTER(C.c_uint64)]),
    'pgx_first_insertions': (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    'pgx_format_labels': (C.c_int, [_S, _S, _P, _P, C.c_uint64, C.c_uint32, _P]),
    'pgx_format_labels_ucs4': (C.c_int, [_S, _S, _P, _P, C.c_uint64, C.c_uint32, _P]),
    'pgx_fasta_write_clustered': (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _S, _S, _S, _S, _S]),
    'pgx_version': (C.c_int, []),
    'pgx_last_error': (C.c_char_p, []),
    'pgx_ctx_create': (C.c_int, [C.c_int, C.POINTER(_P)]),
    'pgx_ctx_create_on': (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(_P)]),
    'pgx_ctx_destroy': (None, [_P]),
    'pgx_device_info': (C.c_int, [_P, C.POINTER(DeviceInfo)]),
    'pgx_profile_enable': (C.c_int, [_P, C.c_int]),
    'pgx_profile_reset': (C.c_int, [_P]),
    'pgx_profile_count': (C.c_int, [_P]),
    'pgx_profile_read': (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double),
                                   C.POINTER(C.c_uint64)]),
    'pgx_bitmap_stride_words': (C.c_uint32, [C.c_uint32]),
    'pgx_presence_bitmap': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_uint64)]),
    'pgx_presence_bitmap_dev': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P]),
    'pgx_pan_core_coo': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P,
                                   C.POINTER(C.c_uint64)]),
    'pgx_pan_core': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P]),
    'pgx_row_counts': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_uint64)]),
    'pgx_row_counts_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    'pgx_heaps_fit': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    'pgx_heaps_fit_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    'pgx_pan_core_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    'pgx_pan_core_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P,
                                   C.c_size_t, _P]),
    'pgx_bernoulli_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'pgx_bernoulli_eval_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, C.c_size_t, _P]),
    'pgx_bernoulli_load': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    'pgx_bernoulli_load_resident': (C.c_int, [_P, C.c_uint64, _P, C.c_uint32, C.c_uint32]),
    'pgx_bernoulli_eval': (C.c_int, [_P, _P, C.c_uint32, _P]),
    'pgx_bernoulli_cd_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'pgx_bernoulli_cd_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_double, C.c_double, C.c_double, C.c_uint32,
                                       C.c_uint32, _P, _P, _P, C.c_size_t, _P]),
    'pgx_bernoulli_cd': (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32, _P, _P]),
    'pgx_bernoulli_cd_stats': (C.c_int, [_P, _P]),
    'pgx_bbn_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'pgx_bbn_ks_sim_dev': (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.c_size_t, _P]),
    'pgx_bbn_ks_sim': (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_int32),
                                 C.c_uint64, _P]),
    'pgx_bbn_draws': (C.c_int, [_P, _P, C.c_uint32, C.c_uint64, _P, C.POINTER(C.c_int32), C.c_uint64, _P]),
    'pgx_fcd_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'pgx_fcd': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _P, C.POINTER(FcdInfo),
                          C.POINTER(C.c_uint64)]),
    'pgx_fcd_resident': (C.c_int, [_P, C.c_uint64, _P, _P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _P,
                                   C.POINTER(FcdInfo)]),
    'pgx_fcd_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _P, _P, C.c_size_t, _P,
                              C.POINTER(FcdInfo)]),
    'pgx_fcd_fetch': (C.c_int, [_P, _P, _P, _P, _P, _P]),
    'pgx_fcd_coverage': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_uint64, _P,
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    'pgx_fcd_match_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]),
    'pgx_fcd_match': (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint64, _P, _P,
                                C.POINTER(C.c_uint64), _P]),
    'pgx_fcd_match_dev': (C.c_int, [_P, _P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P,
                                    C.c_size_t, _P]),
    'pgx_assoc_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'pgx_assoc': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P,
                            _P, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    'pgx_assoc_resident': (C.c_int, [_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32,
                                     _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    'pgx_assoc_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P,
                                C.c_size_t, _P, C.POINTER(C.c_uint32)]),
    'pgx_svm_bag_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    'pgx_svm_bag': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P,
                              C.c_double, C.c_uint32, _P, _P, _P, _P, _P]),
    'pgx_svm_bag_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, C.c_double,
                                  C.c_uint32, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    'pgx_allele_runs_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    'pgx_allele_runs': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint32,
                                  _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'pgx_allele_runs_dev': (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P, _P, _P,
                                      _P, _P, _P, C.c_size_t, _P]),
    'pgx_core_select_block': (C.c_uint32, []),
    'pgx_core_select_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    'pgx_core_select': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint32,
                                  _P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P]),
    'pgx_core_select_dev': (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P,
                                      _P, _P, _P, _P, _P, C.c_size_t, _P]),
    'pgx_window_scan_tile': (C.c_uint32, []),
    'pgx_window_scan_workspace_bytes': (C.c_size_t, [C.c_uint64, C.c_uint32, C.c_uint32]),
    'pgx_window_scan': (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    'pgx_window_scan_dev': (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.c_size_t, _P]),
    'pgx_dict_group_bytes': (C.c_uint32, []),
    'pgx_dict_workspace_bytes': (C.c_size_t, [C.c_uint64, C.c_uint32]),
    'pgx_dict_load': (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P]),
    'pgx_dict_query': (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    'pgx_dict_match_dev': (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t, _P]),
    'pgx_prox_cut_group_bytes': (C.c_uint32, []),
    'pgx_prox_group_tile': (C.c_uint32, []),
    'pgx_prox_group_workspace_bytes': (C.c_size_t, [C.c_uint32]),
    'pgx_prox_cut': (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint32, _P, _P]),
    'pgx_prox_cut_dev': (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint32, _P, _P, _P]),
    'pgx_prox_group': (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    'pgx_prox_group_dev': (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_size_t, _P]),
    'pgx_annot_row_tile': (C.c_uint32, []),
    'pgx_annot_run_tile': (C.c_uint32, []),
    'pgx_annot_vote_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint64, C.c_uint32]),
    'pgx_annot_vote': (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P]),
    'pgx_annot_vote_dev': (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P,
                                     C.c_size_t, _P]),
    'pgx_graph_reach_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    'pgx_graph_reach': (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _P, _P]),
    'pgx_graph_reach_dev': (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint64, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P,
                                      C.c_size_t, _P]),
    'pgx_term_scan_group_bytes': (C.c_uint32, []),
    'pgx_term_scan': (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, _P]),
    'pgx_term_scan_dev': (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint64, C.c_uint32, _P,
                                    _P]),
    'pgx_tuple_group_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'pgx_tuple_group': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P]),
    'pgx_tuple_group_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_size_t, _P]),
    'pgx_mic_infer': (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P,
                                _P, _P, C.c_uint64, _P]),
    'pgx_mic_infer_dev': (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P,
                                    _P, _P, _P, C.c_uint64, _P, _P]),
    'pgx_tree_content_stride': (C.c_uint32, [C.c_uint32]),
    'pgx_tree_content_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint64]),
    'pgx_tree_content': (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P,
                                   _P, C.POINTER(C.c_uint64)]),
    'pgx_tree_content_dev': (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint32, C.c_uint64, _P, _P, C.c_uint32, _P,
                                       _P, _P, C.c_size_t, _P]),
    'pgx_pattern_scan_tile': (C.c_uint32, []),
    'pgx_pattern_workspace_bytes': (C.c_size_t, [C.c_uint64, C.c_uint32]),
    'pgx_pattern_load': (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32]),
    'pgx_pattern_query': (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    'pgx_pattern_scan_dev': (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_size_t,
                                       _P]),
    'pgx_near_scan_tile': (C.c_uint32, []),
    'pgx_near_workspace_bytes': (C.c_size_t, [C.c_uint64, C.c_uint32, C.c_uint64]),
    'pgx_near_load': (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32]),
    'pgx_near_query': (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, _P, _P]),
    'pgx_near_scan_dev': (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint64, C.c_uint32,
                                    _P, _P, _P, C.c_size_t, _P]),
    'pgx_sw_max_length': (C.c_uint32, []),
    'pgx_sw_strip_width': (C.c_uint32, []),
    'pgx_sw_round_pairs': (C.c_uint32, [_P, C.c_int]),
    'pgx_sw_workspace_bytes': (C.c_size_t, [_P, C.c_uint32, C.c_uint32]),
    'pgx_sw_last_stats_pairs': (C.c_uint32, [_P]),
    'pgx_sw_pairs': (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P]),
    'pgx_sw_pairs_dev': (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _P,
                                   C.c_size_t, _P]),
    'pgx_genome_sets_diff':(C.c_int, [_P, _P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P]),
    'pgx_genome_sets_diff_dev': (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    'pgx_cluster_greedy': (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(ClusterParams), _P, _P, _P, _P,
                                     C.POINTER(C.c_uint32), C.POINTER(ClusterStats)]),
    'pgx_cluster_window_cap': (C.c_uint32, [C.POINTER(ClusterParams)]),
    'pgx_rccl_load': (C.c_int, [_S]),
    'pgx_rccl_unique_id': (C.c_int, [_P]),
    'pgx_rccl_comm_create': (C.c_int, [_P, _P, C.c_int, C.c_int]),
    'pgx_rccl_comm_destroy': (C.c_int, [_P]),
    'pgx_cluster_greedy_dev': (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint64, C.POINTER(ClusterParams), _P, _P,
                                         _P, _P, C.POINTER(C.c_uint32), C.POINTER(ClusterStats), _P]),
}

_lib = None
_lock = threading.Lock()


def _one_hip_runtime():
    """One HIP runtime per process, whatever the import order. PyTorch-ROCm wheels bundle their own
    libamdhip64 under the SAME soname (libamdhip64.so.7) libpgx links to, and the dynamic loader
    binds every later user of that soname to whichever copy was mapped first. With the system copy
    first, a later `import torch` would run on a runtime it was not built for (seen to fail with
    "No HIP GPUs are available"). So: if no libamdhip64 is mapped yet and a torch installation
    exists, its copy is mapped first -- by path, WITHOUT importing torch -- and libpgx, and torch
    whenever it comes, share it. Without torch the system runtime (libpgx's RUNPATH) serves."""
    try:
        with open('/proc/self/maps') as f:
            if 'libamdhip64' in f.read():
                return
    except OSError:
        pass
    if os.environ.get('PGX_HIP_RUNTIME') == 'system':
        return
    try:
        spec = importlib.util.find_spec('torch')     # locates the package, does not import it
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load libpgx.so once; raises PgxError if it has not been built."""
    global _lib
    with _lock:
        if _lib is None:
            _one_hip_runtime()
            if not os.path.exists(_LIB_PATH):
                raise PgxError('%s not found: build it with `python -c "import __graft_entry__ as g; '
                               'g.build()"` or `make -C pangenomix_amd/csrc` (there is no CPU fallback)'
                               % _LIB_PATH)
            handle = C.CDLL(_LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(handle, name)
                fn.restype, fn.argtypes = res, args
            _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        err = PgxError('libpgx error %d: %s' % (rc, lib().pgx_last_error().decode('utf-8', 'replace')))
        err.status = rc
        raise err


ERR_NOMEM = -4   # PGX_ERR_NOMEM


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rccl_path():
    """The librccl.so this process should share: PyTorch-ROCm's bundled copy when there is one (found by path, without
    importing torch), else whatever the loader finds. PGX_RCCL_LIB overrides."""
    env = os.environ.get('PGX_RCCL_LIB')
    if env:
        return env
    import importlib.util
    spec = importlib.util.find_spec('torch')
    if spec and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'librccl.so')
        if os.path.exists(cand):
            return cand
    return 'librccl.so'


def rccl_load(path=None):
    check(lib().pgx_rccl_load((path or rccl_path()).encode()))


def rccl_unique_id():
    rccl_load()
    buf = (C.c_uint8 * 128)()
    check(lib().pgx_rccl_unique_id(C.cast(buf, _P)))
    return bytes(buf)


def _legacy_key(key):
    if not (isinstance(key, np.ndarray) and key.dtype == np.uint32 and key.shape == (624,) and key.flags.c_contiguous):
        raise ValueError('key must be a C-contiguous uint32[624] array')
    return key


def legacy_uniform_words(key, pos, n_words):
    """(words uint32[n_words], pos): the next raw outputs of numpy's legacy generator from state (key, pos); key
    (uint32[624], C-contiguous) is advanced IN PLACE. Host only: needs the library, not a device."""
    _legacy_key(key)
    out = np.empty(int(n_words), dtype=np.uint32)
    p = C.c_int32(int(pos))
    check(lib().pgx_legacy_uniform_words(_ptr(key), C.byref(p), int(n_words), _ptr(out)))
    return out, int(p.value)


def _bbn_args(draw_cdf, key, pos):
    draw_cdf = np.ascontiguousarray(draw_cdf, dtype=np.float64)
    if draw_cdf.ndim != 1 or draw_cdf.size == 0:
        raise ValueError('draw_cdf must be a non-empty 1-D array')
    return draw_cdf, _legacy_key(key), C.c_int32(int(pos))


def _coo_args(rows, genomes):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    genomes = np.ascontiguousarray(genomes, dtype=np.int32)
    if rows.shape != genomes.shape or rows.ndim != 1:
        raise ValueError('rows and genomes must be 1-D arrays of equal length')
    return rows, genomes


class Context(object):
    """Owns a pgx_ctx (device state). One per thread; not re-entrant."""

    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        check(lib().pgx_ctx_create(int(device_id), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().pgx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def device_info(self):
        info = DeviceInfo()
        check(lib().pgx_device_info(self._h, C.byref(info)))
        return {'name': info.name.decode(), 'arch': info.arch.decode(), 'device_id': info.device_id,
                'compute_units': info.compute_units, 'wavefront_size': info.wavefront_size,
                'lds_bytes_per_block': info.lds_bytes_per_block, 'hbm_bytes': info.hbm_bytes,
                'clock_khz': info.clock_khz}

    # -- the library's own RCCL communicator (record-sharded mode without a callback) ----------
    def comm_create(self, unique_id, rank, world):
        """Collective: every process calls it with the same 128-byte id (rccl_unique_id() of one of them)."""
        uid = bytes(unique_id)
        if len(uid) != 128:
            raise ValueError('the RCCL unique id is 128 bytes')
        rccl_load()
        check(lib().pgx_rccl_comm_create(self._h, C.cast(C.c_char_p(uid), _P), int(rank), int(world)))
        self.comm = (int(rank), int(world))

    def comm_destroy(self):
        check(lib().pgx_rccl_comm_destroy(self._h))
        self.comm = None

    comm = None

    # -- per-kernel timing ---------------------------------------------------
    def profile(self, on=True):
        check(lib().pgx_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        check(lib().pgx_profile_reset(self._h))

    def profile_read(self):
        """{kernel name: (total_ms, launches)}; waits for pending events."""
        out = {}
        for slot in range(lib().pgx_profile_count(self._h)):
            name = C.create_string_buffer(64)
            ms, n = C.c_double(0), C.c_uint64(0)
            check(lib().pgx_profile_read(self._h, slot, name, 64, C.byref(ms), C.byref(n)))
            out[name.value.decode()] = (ms.value, int(n.value))
        return out

    # -- device-resident variants (pointers are raw device addresses, e.g. torch data_ptr) --
    def presence_bitmap_dev(self, d_rows, d_genomes, n_records, n_rows, n_genomes, d_bits, stream=0, d_counters=None):
        check(lib().pgx_presence_bitmap_dev(self._h, d_rows, d_genomes, int(n_records), int(n_rows),
                                            int(n_genomes), d_bits, d_counters, stream))

    def pan_core_dev(self, d_bits, n_genes, n_genomes, d_perms, n_iter, d_pan, d_core, d_ws, ws_bytes, stream=0):
        check(lib().pgx_pan_core_dev(self._h, d_bits, int(n_genes), int(n_genomes), d_perms, int(n_iter),
                                     d_pan, d_core, d_ws, int(ws_bytes), stream))

    def row_counts_dev(self, d_bits, n_rows, n_genomes, d_counts, stream=0):
        check(lib().pgx_row_counts_dev(self._h, d_bits, int(n_rows), int(n_genomes), d_counts, stream))

    def heaps_fit_dev(self, d_pan, n_iter, n_genomes, d_alpha, d_kappa, stream=0):
        """d_pan: int32 [n_iter, n_genomes], e.g. pan_core_dev's output in place."""
        check(lib().pgx_heaps_fit_dev(self._h, d_pan, int(n_iter), int(n_genomes), d_alpha, d_kappa, stream))

    def bernoulli_eval_dev(self, d_bits, n_genes, n_genomes, d_pq, d_out, d_ws, ws_bytes, flags=0, stream=0):
        check(lib().pgx_bernoulli_eval_dev(self._h, d_bits, int(n_genes), int(n_genomes), d_pq, int(flags), d_out, d_ws,
                                           int(ws_bytes), stream))

    def bernoulli_cd_dev(self, d_bits, n_genes, n_genomes, d_init_p, init_q, lo, hi, n_iterations, d_table, d_solver,
                         d_ws, ws_bytes, flags=0, stream=0):
        """d_table, d_solver (or None): float64 [1 + n_genes + n_genomes, n_iterations + 1]; one synchronisation of
        `stream` at the end."""
        check(lib().pgx_bernoulli_cd_dev(self._h, d_bits, int(n_genes), int(n_genomes), d_init_p, float(init_q), float(lo),
                                         float(hi), int(n_iterations), int(flags), d_table, d_solver, d_ws, int(ws_bytes),
                                         stream))

    # -- K3 ----------------------------------------------------------------
    def presence_bitmap(self, rows, genomes, n_rows, n_genomes, return_duplicates=False):
        rows, genomes = _coo_args(rows, genomes)
        stride = lib().pgx_bitmap_stride_words(int(n_rows))
        bits = np.empty((int(n_genomes), stride), dtype=np.uint64)
        dup = C.c_uint64(0)
        check(lib().pgx_presence_bitmap(self._h, _ptr(rows), _ptr(genomes), rows.size,
                                        int(n_rows), int(n_genomes), _ptr(bits), C.byref(dup)))
        return (bits, int(dup.value)) if return_duplicates else bits

    def heaps_fit(self, pan):
        """(alpha, kappa) float64 per row of the pan table [n_iter, n_genomes]."""
        pan = np.ascontiguousarray(pan, dtype=np.float64)
        if pan.ndim != 2:
            raise ValueError('pan must be [n_iter, n_genomes]')
        alpha = np.empty(pan.shape[0], dtype=np.float64)
        kappa = np.empty(pan.shape[0], dtype=np.float64)
        check(lib().pgx_heaps_fit(self._h, _ptr(pan), pan.shape[0], pan.shape[1], _ptr(alpha), _ptr(kappa)))
        return alpha, kappa

    def row_counts(self, rows, genomes, n_rows, n_genomes):
        """(counts int32[n_rows], duplicates): genomes per row, from the device bitmap."""
        rows, genomes = _coo_args(rows, genomes)
        counts = np.empty(int(n_rows), dtype=np.int32)
        dup = C.c_uint64(0)
        check(lib().pgx_row_counts(self._h, _ptr(rows), _ptr(genomes), rows.size, int(n_rows), int(n_genomes),
                                   _ptr(counts), C.byref(dup)))
        return counts, int(dup.value)

    def pan_core_coo(self, rows, genomes, n_genes, n_genomes, perms):
        """(pan, core, duplicates): bitmap built and consumed on the device in one call."""
        rows, genomes = _coo_args(rows, genomes)
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        n_iter = perms.shape[0]
        if perms.ndim != 2 or perms.shape[1] != int(n_genomes):
            raise ValueError('perms must be [n_iter, n_genomes]')
        pan = np.empty((n_iter, int(n_genomes)), dtype=np.int32)
        core = np.empty((n_iter, int(n_genomes)), dtype=np.int32)
        dup = C.c_uint64(0)
        check(lib().pgx_pan_core_coo(self._h, _ptr(rows), _ptr(genomes), rows.size, int(n_genes), int(n_genomes),
                                     _ptr(perms), n_iter, _ptr(pan), _ptr(core), C.byref(dup)))
        return pan, core, int(dup.value)

    def pan_core_table(self, rows, genomes, values, n_genes, n_genomes, n_iter, mt_key, mt_pos):
        """(table float64 [n_iter, 2 n_genomes], duplicates, values that are not 1, perms, new_pos): the whole of
        estimate_pan_core_size() in one library call (pgx.h: pgx_pan_core_table). `values`: the table's stored
        values as int64, or None."""
        rows, genomes = _coo_args(rows, genomes)
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.int64)
            if values.shape != rows.shape:
                raise ValueError('values must match the coordinates')
        perms = np.empty((int(n_iter), int(n_genomes)), dtype=np.int32)
        table = np.empty((int(n_iter), 2 * int(n_genomes)), dtype=np.float64)
        dup, bad, pos = C.c_uint64(0), C.c_uint64(0), C.c_int32(int(mt_pos))
        check(lib().pgx_pan_core_table(self._h, _ptr(rows), _ptr(genomes), _ptr(values), rows.size, int(n_genes),
                                       int(n_genomes), _ptr(mt_key), C.byref(pos), int(n_iter), _ptr(perms), _ptr(table),
                                       C.byref(dup), C.byref(bad)))
        return table, int(dup.value), int(bad.value), perms, int(pos.value)

    # -- device-resident hand-off: clustering result -> bitmap kept in the context -> pan/core curves --------------
    def bitmap_from_clusters(self, cluster_of_group, group_of_record, file_of_record, genome_of_file, n_genes, n_genomes):
        """Build the gene x genome bitmap on the device from a clustering result and keep it there; returns its token
        (pgx.h: pgx_bitmap_from_clusters)."""
        cl = np.ascontiguousarray(cluster_of_group, dtype=np.int32)
        grp = np.ascontiguousarray(group_of_record, dtype=np.int32)
        fil = np.ascontiguousarray(file_of_record, dtype=np.uint32)
        gof = np.ascontiguousarray(genome_of_file, dtype=np.int32)
        if grp.shape != fil.shape:
            raise ValueError('group_of_record and file_of_record must have one entry per record')
        token = C.c_uint64(0)
        check(lib().pgx_bitmap_from_clusters(self._h, _ptr(cl), cl.size, _ptr(grp), _ptr(fil), grp.size, _ptr(gof), gof.size,
                                             int(n_genes), int(n_genomes), C.byref(token)))
        return int(token.value)

    def bitmap_resident_read(self, token, n_genes, n_genomes):
        bits = np.empty((int(n_genomes), lib().pgx_bitmap_stride_words(int(n_genes))), dtype=np.uint64)
        check(lib().pgx_bitmap_resident_read(self._h, int(token), _ptr(bits)))
        return bits

    def pan_core_table_resident(self, token, n_genes, n_genomes, n_iter, mt_key, mt_pos):
        """(table float64 [n_iter, 2 n_genomes], perms, new_pos) from the bitmap that is resident under `token`."""
        perms = np.empty((int(n_iter), int(n_genomes)), dtype=np.int32)
        table = np.empty((int(n_iter), 2 * int(n_genomes)), dtype=np.float64)
        pos = C.c_int32(int(mt_pos))
        check(lib().pgx_pan_core_table_resident(self._h, int(token), int(n_genes), int(n_genomes), _ptr(mt_key), C.byref(pos),
                                                int(n_iter), _ptr(perms), _ptr(table)))
        return table, perms, int(pos.value)

    # -- Bernoulli grid likelihood (compute_bernoulli_grid_core_genome) --------------------------------------------
    def bernoulli_load(self, rows, genomes, n_genes, n_genomes):
        """Upload the binary table's coordinates once; its bitmap stays in the context for bernoulli_eval().
        Returns the number of duplicate coordinates."""
        rows, genomes = _coo_args(rows, genomes)
        dup = C.c_uint64(0)
        check(lib().pgx_bernoulli_load(self._h, _ptr(rows), _ptr(genomes), rows.size, int(n_genes), int(n_genomes),
                                       C.byref(dup)))
        self._bern_shape = (int(n_genes), int(n_genomes))
        return int(dup.value)

    def bernoulli_load_resident(self, token, row_map, n_genomes):
        """Load the table from the bitmap a pipeline left resident under `token`: row i of the table is row
        row_map[i] (its cluster number) of that bitmap. Raises PgxError when the token is stale."""
        row_map = np.ascontiguousarray(row_map, dtype=np.int32)
        self._bern_shape = None
        check(lib().pgx_bernoulli_load_resident(self._h, int(token), _ptr(row_map), row_map.size, int(n_genomes)))
        self._bern_shape = (row_map.size, int(n_genomes))

    def bernoulli_eval(self, pq, exact=False):
        """[LL, dL/dp..., dL/dq...] (float64) of the loaded table at pq = [P; Q]. exact=True: every present cell's
        own log (pgx.h: PGX_BERNOULLI_EXACT)."""
        shape = getattr(self, '_bern_shape', None)
        if shape is None:
            raise PgxError('no table loaded (bernoulli_load / bernoulli_load_resident)')
        pq = np.ascontiguousarray(pq, dtype=np.float64)
        if pq.shape != (shape[0] + shape[1],):
            raise ValueError('pq must hold n_genes + n_genomes values')
        out = np.empty(pq.size + 1, dtype=np.float64)
        check(lib().pgx_bernoulli_eval(self._h, _ptr(pq), 1 if exact else 0, _ptr(out)))
        return out

    def bernoulli_cd(self, init_p, init_q, lo, hi, n_iterations, use_logs=False, solver_table=False):
        """Coordinate descent on the loaded table (pgx.h: pgx_bernoulli_cd): the float64 table
        [1 + n_genes + n_genomes, n_iterations + 1] (row 0 = LL, column 0 = the start point), and with solver_table=True
        also the same table in the solver's own variables (logs when use_logs). init_p: n_genes values inside [lo, hi].
        A solve that does not converge raises PgxError (a RuntimeError)."""
        shape = getattr(self, '_bern_shape', None)
        if shape is None:
            raise PgxError('no table loaded (bernoulli_load / bernoulli_load_resident)')
        init_p = np.ascontiguousarray(init_p, dtype=np.float64)
        if init_p.shape != (shape[0],):
            raise ValueError('init_p must hold n_genes values')
        n_iterations = int(n_iterations)
        if n_iterations < 0:
            raise ValueError('n_iterations must not be negative')
        table = np.empty((1 + shape[0] + shape[1], n_iterations + 1), dtype=np.float64)
        solver = np.empty_like(table) if solver_table else None
        check(lib().pgx_bernoulli_cd(self._h, _ptr(init_p), float(init_q), float(lo), float(hi), n_iterations,
                                     BERNOULLI_CD_LOGS if use_logs else 0, _ptr(table), _ptr(solver)))
        return (table, solver) if solver_table else table

    def bernoulli_cd_stats(self):
        """Of the last bernoulli_cd / bernoulli_cd_dev: evaluations of f, most evaluations in one solve, solves that
        did not converge, solves."""
        out = np.zeros(4, dtype=np.uint64)
        check(lib().pgx_bernoulli_cd_stats(self._h, _ptr(out)))
        return {'evaluations': int(out[0]), 'max_evaluations': int(out[1]), 'not_converged': int(out[2]),
                'solves': int(out[3])}

    # -- Monte-Carlo KS test of a beta-binomial fit (ks_montecarlo_bbn / draw_bbn) -------------------------------------
    def bbn_ks_sim(self, draw_cdf, model_cdf, n_samples, iterations, key, pos, chunk_draws=0):
        """(ks_sim float64[iterations], pos): the KS statistic of every iteration's n_samples draws from the legacy
        generator state (key uint32[624], advanced IN PLACE; pos), as pgx.h's pgx_bbn_ks_sim states it."""
        draw_cdf, key, p = _bbn_args(draw_cdf, key, pos)
        model_cdf = np.ascontiguousarray(model_cdf, dtype=np.float64)
        if model_cdf.shape != draw_cdf.shape:
            raise ValueError('draw_cdf and model_cdf must have the same length')
        out = np.empty(int(iterations), dtype=np.float64)
        check(lib().pgx_bbn_ks_sim(self._h, _ptr(draw_cdf), _ptr(model_cdf), draw_cdf.size, int(n_samples),
                                   int(iterations), _ptr(key), C.byref(p), int(chunk_draws), _ptr(out)))
        return out, int(p.value)

    def bbn_ks_sim_dev(self, d_words, d_draw_cdf, d_model_cdf, sim_limit, n_samples, iterations, d_ks_sim, d_ws,
                       ws_bytes, stream=0):
        check(lib().pgx_bbn_ks_sim_dev(self._h, d_words, d_draw_cdf, d_model_cdf, int(sim_limit), int(n_samples),
                                       int(iterations), d_ks_sim, d_ws, int(ws_bytes), stream))

    def bbn_draws(self, draw_cdf, size, key, pos, chunk_draws=0):
        """(values int64[size], pos): searchsorted(draw_cdf, random_sample(size), side='right') from the legacy
        generator state (key advanced IN PLACE)."""
        draw_cdf, key, p = _bbn_args(draw_cdf, key, pos)
        out = np.empty(int(size), dtype=np.int64)
        check(lib().pgx_bbn_draws(self._h, _ptr(draw_cdf), draw_cdf.size, int(size), _ptr(key), C.byref(p),
                                  int(chunk_draws), _ptr(out)))
        return out, int(p.value)

    # -- formal concept decomposition (fcd.formal_concept_decomposition / compute_concept_coverage) --------------------
    @staticmethod
    def _fcd_args(n_genomes, limit, overlap, dim_factors):
        flags = FCD_OVERLAP if overlap else 0
        if dim_factors is not None:
            dim_factors = np.ascontiguousarray(dim_factors, dtype=np.float64)
            if dim_factors.shape != (int(n_genomes),):
                raise ValueError('dim_factors must hold one factor per genome')
            flags |= FCD_DIM_BALANCE
        if not 0 <= int(limit) < 2 ** 64:
            raise ValueError('limit out of range')
        return flags, dim_factors

    def _fcd_fetch(self, info):
        """The concepts of the run that has just ended: {'rows', 'row_offsets', 'cols', 'col_offsets' (a concept's rows
        ascending / its columns in the order they joined, end to end, and n + 1 offsets), 'left' (ones uncovered after
        each concept), 'steps', 'ones_total', 'ones_left'}."""
        n = int(info.n_concepts)
        out = {'rows': np.empty(int(info.n_row_entries), dtype=np.int32), 'row_offsets': np.empty(n + 1, dtype=np.uint64),
               'cols': np.empty(int(info.n_col_entries), dtype=np.int32), 'col_offsets': np.empty(n + 1, dtype=np.uint64),
               'left': np.empty(n, dtype=np.uint64)}
        check(lib().pgx_fcd_fetch(self._h, _ptr(out['rows']), _ptr(out['row_offsets']), _ptr(out['cols']),
                                  _ptr(out['col_offsets']), _ptr(out['left'])))
        out.update(steps=int(info.steps), ones_total=int(info.ones_total), ones_left=int(info.ones_left))
        return out

    def fcd(self, rows, genomes, n_rows, n_genomes, limit, overlap=False, dim_factors=None):
        """(concepts, duplicates) of the binary table with the given COO coordinates (pgx.h: pgx_fcd + pgx_fcd_fetch);
        with duplicate coordinates nothing is decomposed and concepts is None."""
        rows, genomes = _coo_args(rows, genomes)
        flags, dim_factors = self._fcd_args(n_genomes, limit, overlap, dim_factors)
        info, dup = FcdInfo(), C.c_uint64(0)
        check(lib().pgx_fcd(self._h, _ptr(rows), _ptr(genomes), rows.size, int(n_rows), int(n_genomes), int(limit), flags,
                            _ptr(dim_factors), C.byref(info), C.byref(dup)))
        if dup.value:
            return None, int(dup.value)
        return self._fcd_fetch(info), 0

    def fcd_resident(self, token, row_map, col_map, n_genomes, limit, overlap=False, dim_factors=None):
        """The same from the bitmap a pipeline left resident under `token` (not modified): row i / column j of the table is
        row row_map[i] / column col_map[j] (None: j) of it. Raises PgxError when the token is stale."""
        row_map = np.ascontiguousarray(row_map, dtype=np.int32)
        if col_map is not None:
            col_map = np.ascontiguousarray(col_map, dtype=np.int32)
            if col_map.shape != (int(n_genomes),):
                raise ValueError('col_map must hold one entry per genome')
        flags, dim_factors = self._fcd_args(n_genomes, limit, overlap, dim_factors)
        info = FcdInfo()
        check(lib().pgx_fcd_resident(self._h, int(token), _ptr(row_map), _ptr(col_map), row_map.size, int(n_genomes),
                                     int(limit), flags, _ptr(dim_factors), C.byref(info)))
        return self._fcd_fetch(info)

    def fcd_dev(self, d_bits, n_rows, n_genomes, limit, d_ws, ws_bytes, overlap=False, dim_factors=None, stream=0):
        """The same on a bitmap in device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        flags, dim_factors = self._fcd_args(n_genomes, limit, overlap, dim_factors)
        info = FcdInfo()
        check(lib().pgx_fcd_dev(self._h, d_bits, int(n_rows), int(n_genomes), int(limit), flags, _ptr(dim_factors), d_ws,
                                int(ws_bytes), stream, C.byref(info)))
        return self._fcd_fetch(info)

    def fcd_coverage(self, rows, genomes, n_rows, n_genomes, concept_rows, row_offsets, concept_cols, col_offsets):
        """(cleared uint64[n_concepts], ones, duplicates): the ones each concept clears when they are cleared from the
        table one after the other, and the ones of the table (pgx.h: pgx_fcd_coverage)."""
        rows, genomes = _coo_args(rows, genomes)
        concept_rows = np.ascontiguousarray(concept_rows, dtype=np.int32)
        concept_cols = np.ascontiguousarray(concept_cols, dtype=np.int32)
        row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        col_offsets = np.ascontiguousarray(col_offsets, dtype=np.uint64)
        n = row_offsets.size - 1
        if n < 0 or col_offsets.size != n + 1 or (n and (int(row_offsets[n]) != concept_rows.size
                                                         or int(col_offsets[n]) != concept_cols.size)):
            raise ValueError('offsets do not match the concept arrays')
        cleared = np.zeros(max(n, 0), dtype=np.uint64)
        ones, dup = C.c_uint64(0), C.c_uint64(0)
        check(lib().pgx_fcd_coverage(self._h, _ptr(rows), _ptr(genomes), rows.size, int(n_rows), int(n_genomes),
                                     _ptr(concept_rows), _ptr(row_offsets), _ptr(concept_cols), _ptr(col_offsets), n,
                                     _ptr(cleared), C.byref(ones), C.byref(dup)))
        return cleared, int(ones.value), int(dup.value)

    @staticmethod
    def _fcd_match_sizes(n_rows, n_cols, n1, n2):
        sizes = tuple(int(x) for x in (n_rows, n_cols, n1, n2))
        if not all(0 <= x < 2 ** 32 for x in sizes):           # (the library refuses 2^31 and above with its own message)
            raise ValueError('table or concept list too large')
        return sizes

    def fcd_match(self, n_rows, n_cols, rows1, row_off1, cols1, col_off1, rows2, row_off2, cols2, col_off2, matrix=False):
        """(match int64[k], overlap uint64[k], total, O or None): the greedy pairing of two concept lists of an
        n_rows x n_cols table, each as fcd_coverage takes them (pgx.h: pgx_fcd_match); matrix=True also returns the whole
        n1 x n2 uint64 overlap matrix."""
        fam = []
        for idx, off in ((rows1, row_off1), (cols1, col_off1), (rows2, row_off2), (cols2, col_off2)):
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            if idx.ndim != 1 or off.ndim != 1 or off.size < 1 or int(off[-1]) != idx.size:
                raise ValueError('offsets do not match the concept arrays')
            fam.append((idx, off))
        n1, n2 = fam[0][1].size - 1, fam[2][1].size - 1
        if fam[1][1].size != n1 + 1 or fam[3][1].size != n2 + 1:
            raise ValueError('row and column offsets of a list differ in length')
        n_rows, n_cols, n1, n2 = self._fcd_match_sizes(n_rows, n_cols, n1, n2)
        k = min(n1, n2)
        match, overlap = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.uint64)
        total = C.c_uint64(0)
        O = np.zeros((n1, n2), dtype=np.uint64) if matrix else None
        check(lib().pgx_fcd_match(self._h, n_rows, n_cols, _ptr(fam[0][0]), _ptr(fam[0][1]), _ptr(fam[1][0]), _ptr(fam[1][1]),
                                  n1, _ptr(fam[2][0]), _ptr(fam[2][1]), _ptr(fam[3][0]), _ptr(fam[3][1]), n2, _ptr(match),
                                  _ptr(overlap), C.byref(total), _ptr(O)))
        return match, overlap, int(total.value), O

    def fcd_match_workspace_bytes(self, n_rows, n_cols, n1, n2):
        return int(lib().pgx_fcd_match_workspace_bytes(*self._fcd_match_sizes(n_rows, n_cols, n1, n2)))

    def fcd_match_dev(self, d_row_masks1, d_col_masks1, n1, d_row_masks2, d_col_masks2, n2, n_rows, n_cols, d_match,
                      d_overlap, d_total, d_ws, ws_bytes, d_matrix=None, stream=0):
        """The same on bit masks in device memory (raw device addresses; concept-major, see pgx.h: pgx_fcd_match_dev).
        Nothing is allocated and nothing synchronised: the results are in the caller's buffers in stream order."""
        n_rows, n_cols, n1, n2 = self._fcd_match_sizes(n_rows, n_cols, n1, n2)
        check(lib().pgx_fcd_match_dev(self._h, d_row_masks1, d_col_masks1, n1, d_row_masks2, d_col_masks2, n2, n_rows, n_cols,
                                      d_match, d_overlap, d_total, d_matrix, d_ws, int(ws_bytes), stream))

    # -- association screen (sparse_utils.compress_rows*, ml_pipelines.contingency_tables_from_sparse) -------------------
    @staticmethod
    def _assoc_args(n_rows, n_genomes, col_map, masks, blocks, drop_empty, narrow_hash):
        n_rows, n_genomes = int(n_rows), int(n_genomes)
        if col_map is not None:
            col_map = np.ascontiguousarray(col_map, dtype=np.int32)
            if col_map.ndim != 1:
                raise ValueError('col_map must be 1-D')
        n_sel = n_genomes if col_map is None else int(col_map.size)
        words = max(1, (n_sel + 63) // 64)
        n_targets = 0
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint64)
            if masks.ndim != 2 or masks.shape[1] != words:
                raise ValueError('masks must be [n_targets, %d] words' % words)
            n_targets = int(masks.shape[0])
        flags = ((ASSOC_BLOCKS if blocks else 0) | (ASSOC_DROP_EMPTY if blocks and drop_empty else 0) |
                 (ASSOC_NARROW_HASH if narrow_hash else 0))
        out = {'tp': np.zeros((n_targets, n_rows), dtype=np.uint32), 'incidence': np.zeros(n_rows, dtype=np.uint32),
               'block_of_row': np.full(n_rows if blocks else 0, -1, dtype=np.int32),
               'rep_row': np.zeros(n_rows if blocks else 0, dtype=np.int32)}
        return col_map, n_sel, masks, n_targets, flags, out

    @staticmethod
    def _assoc_out(out, blocks, n_blocks):
        out['rep_row'] = out['rep_row'][:int(n_blocks.value)] if blocks else None
        if not blocks:
            out['block_of_row'] = None
        return out

    def assoc(self, rows, genomes, n_rows, n_genomes, col_map=None, masks=None, blocks=False, drop_empty=False,
              narrow_hash=False):
        """({'tp' uint32 [n_targets, n_rows], 'incidence' uint32 [n_rows], 'block_of_row' int32 [n_rows], 'rep_row' int32
        [n_blocks]}, duplicates) of the binary table with the given COO coordinates, restricted to the genomes col_map
        (pgx.h: pgx_assoc); with duplicate coordinates nothing is computed and the dict is None. narrow_hash: the test seam
        ASSOC_NARROW_HASH."""
        rows, genomes = _coo_args(rows, genomes)
        col_map, n_sel, masks, n_targets, flags, out = self._assoc_args(n_rows, n_genomes, col_map, masks, blocks, drop_empty,
                                                                        narrow_hash)
        n_blocks, dup = C.c_uint32(0), C.c_uint64(0)
        check(lib().pgx_assoc(self._h, _ptr(rows), _ptr(genomes), rows.size, int(n_rows), int(n_genomes), _ptr(col_map), n_sel,
                              _ptr(masks), n_targets, flags, _ptr(out['tp']), _ptr(out['incidence']),
                              _ptr(out['block_of_row']), _ptr(out['rep_row']), C.byref(n_blocks), C.byref(dup)))
        if dup.value:
            return None, int(dup.value)
        return self._assoc_out(out, blocks, n_blocks), 0

    def assoc_resident(self, token, row_map, n_genomes, col_map=None, masks=None, blocks=False, drop_empty=False,
                       narrow_hash=False):
        """The same from the bitmap a pipeline left resident under `token` (not modified): row i of the table is row
        row_map[i] of it. Raises PgxError when the token is stale."""
        row_map = np.ascontiguousarray(row_map, dtype=np.int32)
        col_map, n_sel, masks, n_targets, flags, out = self._assoc_args(row_map.size, n_genomes, col_map, masks, blocks,
                                                                        drop_empty, narrow_hash)
        n_blocks = C.c_uint32(0)
        check(lib().pgx_assoc_resident(self._h, int(token), _ptr(row_map), row_map.size, int(n_genomes), _ptr(col_map), n_sel,
                                       _ptr(masks), n_targets, flags, _ptr(out['tp']), _ptr(out['incidence']),
                                       _ptr(out['block_of_row']), _ptr(out['rep_row']), C.byref(n_blocks)))
        return self._assoc_out(out, blocks, n_blocks)

    def assoc_dev(self, d_bits, n_rows, n_genomes, d_col_map, n_selected, d_masks, n_targets, d_tp, d_incidence,
                  d_block_of_row, d_rep_row, d_ws, ws_bytes, blocks=True, drop_empty=False, stream=0, narrow_hash=False):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h); returns n_blocks."""
        flags = ((ASSOC_BLOCKS if blocks else 0) | (ASSOC_DROP_EMPTY if blocks and drop_empty else 0) |
                 (ASSOC_NARROW_HASH if narrow_hash else 0))
        n_blocks = C.c_uint32(0)
        check(lib().pgx_assoc_dev(self._h, d_bits, int(n_rows), int(n_genomes), d_col_map, int(n_selected), d_masks,
                                  int(n_targets), flags, d_tp, d_incidence, d_block_of_row, d_rep_row, d_ws, int(ws_bytes),
                                  stream, C.byref(n_blocks)))
        return int(n_blocks.value)

    # -- bagged linear SVMs in the dual (ml_pipelines.BaggedLinearSVC / evaluate_model) ------------------------------------
    SVM_MAX_GENOMES = 4096                   # PGX_SVM_MAX_GENOMES

    def svm_bag(self, rows, genomes, n_rows, n_genomes, masks, mask_of_problem, C_values, multiplicity, labels, tol=1e-10,
                max_steps=0):
        """{'beta' [P, n_genomes], 'coef' [P, n_rows], 'intercept' [P], 'decision' [P, n_genomes] float64, 'steps' uint32 [P]}
        of the P sub-problems {mask_of_problem[p], C_values[p], multiplicity[p]} on the binary table with the given COO
        coordinates (rows = features, genomes = samples), labels uint8 [n_genomes] (pgx.h: pgx_svm_bag). masks: uint64
        [n_masks, stride_words(n_rows)]. max_steps = 0: the library's default."""
        rows, genomes = _coo_args(rows, genomes)
        n_rows, n_genomes = int(n_rows), int(n_genomes)
        stride = int(lib().pgx_bitmap_stride_words(n_rows))
        masks = np.ascontiguousarray(masks, dtype=np.uint64)
        if masks.ndim != 2 or masks.shape[1] != stride:
            raise ValueError('masks must be [n_masks, %d] words' % stride)
        mask_of_problem = np.ascontiguousarray(mask_of_problem, dtype=np.int32)
        C_values = np.ascontiguousarray(C_values, dtype=np.float64)
        multiplicity = np.ascontiguousarray(multiplicity, dtype=np.uint16)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        P = int(mask_of_problem.size)
        if mask_of_problem.ndim != 1 or C_values.shape != (P,) or multiplicity.shape != (P, n_genomes) or \
                labels.shape != (n_genomes,):
            raise ValueError('one mask index, one C and n_genomes multiplicities per sub-problem; one label per genome')
        out = {'beta': np.zeros((P, n_genomes)), 'coef': np.zeros((P, n_rows)), 'intercept': np.zeros(P),
               'decision': np.zeros((P, n_genomes)), 'steps': np.zeros(P, dtype=np.uint32)}
        check(lib().pgx_svm_bag(self._h, _ptr(rows), _ptr(genomes), rows.size, n_rows, n_genomes, _ptr(masks),
                                int(masks.shape[0]), _ptr(mask_of_problem), _ptr(C_values), _ptr(multiplicity), P, _ptr(labels),
                                float(tol), int(max_steps), _ptr(out['beta']), _ptr(out['coef']), _ptr(out['intercept']),
                                _ptr(out['decision']), _ptr(out['steps'])))
        return out

    def svm_bag_workspace_bytes(self, n_rows, n_genomes, n_masks):
        return int(lib().pgx_svm_bag_workspace_bytes(int(n_rows), int(n_genomes), int(n_masks)))

    def svm_bag_dev(self, d_bits, n_rows, n_genomes, d_masks, n_masks, d_mask_of_problem, d_C, d_multiplicity, n_problems,
                    d_labels, d_beta, d_coef, d_intercept, d_decision, d_steps, d_ws, ws_bytes, tol=1e-10, max_steps=0,
                    stream=0):
        """The same on device memory (raw device addresses; synchronises `stream` once at the end, see pgx.h)."""
        check(lib().pgx_svm_bag_dev(self._h, d_bits, int(n_rows), int(n_genomes), d_masks, int(n_masks), d_mask_of_problem,
                                    d_C, d_multiplicity, int(n_problems), d_labels, float(tol), int(max_steps), d_beta,
                                    d_coef, d_intercept, d_decision, d_steps, d_ws, int(ws_bytes), stream))

    # -- runs of allele rows (pangenome.validate_gene_table[_dense], extract_dominant_alleles) -----------------------------
    RUNS_OUTPUTS = ('derived', 'diff', 'diff_per_genome', 'diff_per_run', 'total', 'best_allele', 'best_count')

    @staticmethod
    def _runs_args(run_start, gene_of_run, gene_rows, gene_genomes, want, known, thresholds=()):
        """What allele_runs and core_select (which alone has thresholds) take alike, coerced and checked in the order both
        always did: (run_start, n_runs, gene_of_run, gene COO rows, gene COO genomes, thresholds)."""
        run_start = np.ascontiguousarray(run_start, dtype=np.uint32)
        if run_start.ndim != 1 or run_start.size < 1:
            raise ValueError('run_start must hold n_runs + 1 entries')
        thresholds = np.ascontiguousarray(thresholds, dtype=np.uint32)
        if thresholds.ndim != 1:
            raise ValueError('thresholds must be one-dimensional')
        n_runs = run_start.size - 1
        g_rows = g_genomes = None
        if gene_of_run is not None:
            gene_of_run = np.ascontiguousarray(gene_of_run, dtype=np.int32)
            if gene_of_run.shape != (n_runs,):
                raise ValueError('gene_of_run must hold one entry per run')
            g_rows, g_genomes = _coo_args(gene_rows if gene_rows is not None else [], gene_genomes if gene_genomes is not None else [])
        unknown = set(want) - set(known)
        if unknown:
            raise ValueError('unknown outputs %r' % sorted(unknown))
        return run_start, n_runs, gene_of_run, g_rows, g_genomes, thresholds

    @staticmethod
    def _runs_result(out, dup):
        """(out, (allele duplicates, gene duplicates)); with duplicates nothing was computed and out is None."""
        dups = (int(dup[0]), int(dup[1]))
        return (None if any(dups) else out), dups

    def allele_runs(self, allele_rows, allele_genomes, n_alleles, n_genomes, run_start, gene_rows=None, gene_genomes=None,
                    n_genes=0, gene_of_run=None, want=RUNS_OUTPUTS):
        """({name: array for name in want}, (allele duplicates, gene duplicates)) of the runs [run_start[r], run_start[r + 1])
        of the allele table's rows, compared with rows gene_of_run (-1: none) of the gene table when that is given (pgx.h:
        pgx_allele_runs). 'derived' / 'diff' are uint64 [n_genomes, stride_words(n_runs)] bitmaps, 'diff_per_genome' /
        'diff_per_run' / 'best_count' uint32, 'total' uint64, 'best_allele' int32. With duplicate coordinates nothing is
        computed and the dict is None."""
        a_rows, a_genomes = _coo_args(allele_rows, allele_genomes)
        run_start, n_runs, gene_of_run, g_rows, g_genomes, _ = self._runs_args(run_start, gene_of_run, gene_rows, gene_genomes,
                                                                               want, self.RUNS_OUTPUTS)
        n_genomes = int(n_genomes)
        stride = lib().pgx_bitmap_stride_words(n_runs)
        shapes = {'derived': ((n_genomes, stride), np.uint64), 'diff': ((n_genomes, stride), np.uint64),
                  'diff_per_genome': (n_genomes, np.uint32), 'diff_per_run': (n_runs, np.uint32), 'total': (n_runs, np.uint64),
                  'best_allele': (n_runs, np.int32), 'best_count': (n_runs, np.uint32)}
        out = {k: np.zeros(*shapes[k]) for k in self.RUNS_OUTPUTS if k in want}
        dup = np.zeros(2, dtype=np.uint64)
        check(lib().pgx_allele_runs(self._h, _ptr(a_rows), _ptr(a_genomes), a_rows.size, int(n_alleles), _ptr(g_rows),
                                    _ptr(g_genomes), 0 if g_rows is None else g_rows.size, int(n_genes), n_genomes,
                                    _ptr(run_start), n_runs, _ptr(gene_of_run), *[_ptr(out.get(k)) for k in self.RUNS_OUTPUTS],
                                    _ptr(dup)))
        return self._runs_result(out, dup)

    def allele_runs_dev(self, d_allele_bits, n_alleles, d_gene_bits, n_genes, n_genomes, d_run_start, n_runs, d_gene_of_run,
                        d_derived, d_diff, d_diff_per_genome, d_diff_per_run, d_total, d_best_allele, d_best_count, d_ws,
                        ws_bytes, stream=0):
        """The same on device memory (raw device addresses, None for what is not wanted; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_allele_runs_dev(self._h, d_allele_bits, int(n_alleles), d_gene_bits, int(n_genes), int(n_genomes),
                                        d_run_start, int(n_runs), d_gene_of_run, d_derived, d_diff, d_diff_per_genome,
                                        d_diff_per_run, d_total, d_best_allele, d_best_count, d_ws, int(ws_bytes), stream))

    # -- core / dominant allele selection (core_genome.create_core_genes_fasta, allele_identification.create_alleles_fasta) --
    SELECT_OUTPUTS = ('gene_count', 'best_allele', 'best_count', 'mask', 'selected', 'n_selected')

    def core_select(self, allele_rows, allele_genomes, n_alleles, n_genomes, run_start, thresholds, gene_rows=None,
                    gene_genomes=None, n_genes=0, gene_of_run=None, want=SELECT_OUTPUTS):
        """({name: array for name in want}, (allele duplicates, gene duplicates)) of the runs [run_start[r], run_start[r + 1])
        of the allele table's rows and up to 32 uint32 thresholds (pgx.h: pgx_core_select). 'gene_count' / 'best_count' /
        'mask' are uint32 [n_runs], 'best_allele' int32 [n_runs], 'n_selected' uint32 [n_thresholds]; 'selected' is a list
        of n_thresholds int32 arrays, row t cut to n_selected[t]. With duplicate coordinates nothing is computed and the
        dict is None."""
        a_rows, a_genomes = _coo_args(allele_rows, allele_genomes)
        run_start, n_runs, gene_of_run, g_rows, g_genomes, thresholds = self._runs_args(
            run_start, gene_of_run, gene_rows, gene_genomes, want, self.SELECT_OUTPUTS, thresholds)
        n_thr = thresholds.size
        want = set(want) | ({'n_selected'} if 'selected' in want else set())
        shapes = {'gene_count': (n_runs, np.uint32), 'best_allele': (n_runs, np.int32), 'best_count': (n_runs, np.uint32),
                  'mask': (n_runs, np.uint32), 'selected': ((n_thr, n_runs), np.int32), 'n_selected': (n_thr, np.uint32)}
        out = {k: (np.empty if k == 'selected' else np.zeros)(*shapes[k]) for k in self.SELECT_OUTPUTS if k in want}
        dup = np.zeros(2, dtype=np.uint64)
        check(lib().pgx_core_select(self._h, _ptr(a_rows), _ptr(a_genomes), a_rows.size, int(n_alleles), _ptr(g_rows),
                                    _ptr(g_genomes), 0 if g_rows is None else g_rows.size, int(n_genes), int(n_genomes),
                                    _ptr(run_start), n_runs, _ptr(gene_of_run), _ptr(thresholds), n_thr,
                                    *([_ptr(out.get(k)) for k in self.SELECT_OUTPUTS] + [_ptr(dup)])))
        out, dups = self._runs_result(out, dup)
        if out is not None and 'selected' in out:
            out['selected'] = [out['selected'][t, :int(out['n_selected'][t])].copy() for t in range(n_thr)]
        return out, dups

    def core_select_dev(self, d_allele_bits, n_alleles, d_gene_bits, n_genes, n_genomes, d_run_start, n_runs, d_gene_of_run,
                        d_thresholds, n_thresholds, d_gene_count, d_best_allele, d_best_count, d_mask, d_selected,
                        d_n_selected, d_ws, ws_bytes, stream=0):
        """The same on device memory (raw device addresses, None for what is not wanted; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_core_select_dev(self._h, d_allele_bits, int(n_alleles), d_gene_bits, int(n_genes), int(n_genomes),
                                        d_run_start, int(n_runs), d_gene_of_run, d_thresholds, int(n_thresholds), d_gene_count,
                                        d_best_allele, d_best_count, d_mask, d_selected, d_n_selected, d_ws, int(ws_bytes),
                                        stream))

    # -- fixed-length keys in a text (pangenome.validate_proximal_table_direct) ---------------------------------------------
    def window_scan(self, text, keys, flags=0):
        """found uint8 [n_keys]: 1 where the row of `keys` (uint8 [n_keys, window]) occurs anywhere in `text` (bytes or a
        1-D uint8 array), compared byte by byte (pgx.h: pgx_window_scan). flags: SCAN_NARROW_HASH, the test seam."""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(text, dtype=np.uint8)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        if text.ndim != 1 or keys.ndim != 2:
            raise ValueError('text must be 1-D and keys [n_keys, window]')
        found = np.zeros(keys.shape[0], dtype=np.uint8)
        check(lib().pgx_window_scan(self._h, _ptr(text), text.size, _ptr(keys), keys.shape[0], keys.shape[1], int(flags),
                                    _ptr(found)))
        return found

    def window_scan_dev(self, d_text, text_bytes, d_keys, n_keys, window, d_found, d_ws, ws_bytes, flags=0, stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_window_scan_dev(self._h, d_text, int(text_bytes), d_keys, int(n_keys), int(window), int(flags), d_found,
                                        d_ws, int(ws_bytes), stream))

    # -- whole strings in a set of strings (pangenome.validate_table_against_fasta) -----------------------------------------
    @staticmethod
    def _string_args(blob, offsets):
        if isinstance(blob, (bytes, bytearray, memoryview)):
            blob = np.frombuffer(blob, dtype=np.uint8)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if blob.ndim != 1 or offsets.ndim != 1 or offsets.size < 1:
            raise ValueError('a blob must be 1-D and offsets hold n + 1 entries')
        if int(offsets[-1]) > blob.size:
            raise ValueError('offsets run past the end of the blob')
        return blob, offsets

    def dict_load(self, keys, key_offsets, flags=0, want_first=True):
        """Loads the keys -- key i is the bytes keys[key_offsets[i]:key_offsets[i + 1]] -- for dict_query, replacing an
        earlier set. Returns first int32 [n_keys]: the smallest index of a key with key i's bytes (pgx.h: pgx_dict_load), or
        None if not wanted. flags: DICT_NARROW_HASH, the test seam."""
        keys, key_offsets = self._string_args(keys, key_offsets)
        first = np.zeros(key_offsets.size - 1, dtype=np.int32) if want_first else None
        check(lib().pgx_dict_load(self._h, _ptr(keys), _ptr(key_offsets), key_offsets.size - 1, int(flags), _ptr(first)))
        return first

    def dict_query(self, queries, query_offsets):
        """last int32 [n_queries]: the largest index of a loaded key with the query's bytes, -1 for none."""
        queries, query_offsets = self._string_args(queries, query_offsets)
        last = np.zeros(query_offsets.size - 1, dtype=np.int32)
        check(lib().pgx_dict_query(self._h, _ptr(queries), _ptr(query_offsets), query_offsets.size - 1, _ptr(last)))
        return last

    def dict_match_dev(self, d_keys, d_key_offsets, n_keys, d_queries, d_query_offsets, n_queries, d_out_first, d_out_last,
                       d_ws, ws_bytes, flags=0, stream=0):
        """Both on device memory (raw device addresses, None for no first; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_dict_match_dev(self._h, d_keys, d_key_offsets, int(n_keys), d_queries, d_query_offsets, int(n_queries),
                                       int(flags), d_out_first, d_out_last, d_ws, int(ws_bytes), stream))

    # -- variable-length patterns in a text, with positions and counts (pangenomix_amd.mlst) --------------------------------
    def pattern_load(self, patterns, pattern_offsets, seed, flags=0):
        """Loads the patterns -- pattern k is the bytes patterns[pattern_offsets[k]:pattern_offsets[k + 1]] -- for
        pattern_query, replacing an earlier set. seed: the leading bytes that are hashed, 1..64 and no longer than the shortest
        pattern (pgx.h: pgx_pattern_load). flags: PATTERN_NARROW_HASH, the test seam. Returns the number of patterns."""
        patterns, pattern_offsets = self._string_args(patterns, pattern_offsets)
        check(lib().pgx_pattern_load(self._h, _ptr(patterns), _ptr(pattern_offsets), pattern_offsets.size - 1, int(seed),
                                     int(flags)))
        self._pattern_count = pattern_offsets.size - 1
        return self._pattern_count

    def pattern_query(self, text):
        """(first, count) uint32 [n_patterns] of the loaded patterns in `text` (bytes or a 1-D uint8 array): the smallest
        position of an occurrence, 0xFFFFFFFF for none, and the number of occurrences (pgx.h: pgx_pattern_query)."""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(text, dtype=np.uint8)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        if text.ndim != 1:
            raise ValueError('text must be 1-D')
        n = getattr(self, '_pattern_count', 0)
        first, count = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        check(lib().pgx_pattern_query(self._h, _ptr(text), text.size, _ptr(first), _ptr(count)))
        return first, count

    def pattern_scan_dev(self, d_text, text_bytes, d_patterns, d_pattern_offsets, n_patterns, seed, d_first, d_count, d_ws,
                         ws_bytes, flags=0, stream=0):
        """Load and query in one on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_pattern_scan_dev(self._h, d_text, int(text_bytes), d_patterns, d_pattern_offsets, int(n_patterns),
                                         int(seed), int(flags), d_first, d_count, d_ws, int(ws_bytes), stream))

    # -- variable-length patterns in a text within a number of mismatches (pangenomix_amd.mlst, novel alleles) ----------------
    def near_load(self, patterns, pattern_offsets, max_mismatch, block, flags=0):
        """Loads the patterns for near_query, replacing an earlier set. max_mismatch: uint8 [n_patterns]; block: the bytes of
        an indexed block, 1..64, with (max_mismatch[k] + 1) * block <= the length of pattern k (pgx.h: pgx_near_load). flags:
        NEAR_NARROW_HASH, the test seam. Returns the number of patterns."""
        patterns, pattern_offsets = self._string_args(patterns, pattern_offsets)
        n = pattern_offsets.size - 1
        if np.size(max_mismatch) and (np.min(max_mismatch) < 0 or np.max(max_mismatch) > 255):
            raise ValueError('max_mismatch must be 0..255')
        max_mismatch = np.ascontiguousarray(max_mismatch, dtype=np.uint8)
        if max_mismatch.shape != (n,):
            raise ValueError('max_mismatch must hold one entry per pattern')
        check(lib().pgx_near_load(self._h, _ptr(patterns), _ptr(pattern_offsets), n, _ptr(max_mismatch), int(block), int(flags)))
        self._near_count = n
        return n

    def near_query(self, text, separator=NEAR_NO_SEPARATOR, active=None):
        """best uint64 [n_patterns] of the loaded patterns in `text` (bytes or a 1-D uint8 array): mismatches << 32 | position
        of the best window within max_mismatch, all-ones for none and for a pattern whose `active` (uint8 [n_patterns], None:
        all) is 0 (pgx.h: pgx_near_query)."""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(text, dtype=np.uint8)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        if text.ndim != 1:
            raise ValueError('text must be 1-D')
        n = getattr(self, '_near_count', 0)
        if active is not None:
            active = np.ascontiguousarray(active, dtype=np.uint8)
            if active.shape != (n,):
                raise ValueError('active must hold one entry per pattern')
        best = np.zeros(n, dtype=np.uint64)
        check(lib().pgx_near_query(self._h, _ptr(text), text.size, int(separator), _ptr(active), _ptr(best)))
        return best

    def near_scan_dev(self, d_text, text_bytes, separator, d_patterns, d_pattern_offsets, n_patterns, d_max_mismatch, block,
                      n_blocks, d_active, d_best, d_ws, ws_bytes, flags=0, stream=0):
        """Load and query in one on device memory (raw device addresses, None for no active; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_near_scan_dev(self._h, d_text, int(text_bytes), int(separator), d_patterns, d_pattern_offsets,
                                      int(n_patterns), d_max_mismatch, int(block), int(n_blocks), int(flags), d_active, d_best,
                                      d_ws, int(ws_bytes), stream))

    # -- local alignment of pairs (pangenomix_amd.ncbi.bidirectional_blast) -------------------------------------------------
    def sw_pairs(self, residues1, offsets1, residues2, offsets2, pair_a, pair_b, min_score):
        """out int32 [n_pairs, 8] = score, q_start, q_end, s_start, s_end, n_ident, n_cols, n_gapopen of the best local
        alignment of sequence pair_a[p] of set 1 with sequence pair_b[p] of set 2 (pgx.h: pgx_sw_pairs); the five statistics
        are 0 where score < min_score[p] (int32 [n_pairs], or one number for all) or score is 0."""
        residues1, offsets1 = self._string_args(residues1, offsets1)
        residues2, offsets2 = self._string_args(residues2, offsets2)
        pair_a = np.ascontiguousarray(pair_a, dtype=np.uint32)
        pair_b = np.ascontiguousarray(pair_b, dtype=np.uint32)
        if pair_a.ndim != 1 or pair_a.shape != pair_b.shape:
            raise ValueError('pair_a and pair_b must be 1-D arrays of equal length')
        min_score = np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, dtype=np.int32), pair_a.shape))
        out = np.zeros((pair_a.size, 8), dtype=np.int32)
        check(lib().pgx_sw_pairs(self._h, _ptr(residues1), _ptr(offsets1), offsets1.size - 1, _ptr(residues2), _ptr(offsets2),
                                 offsets2.size - 1, _ptr(pair_a), _ptr(pair_b), pair_a.size, _ptr(min_score), _ptr(out)))
        return out

    def sw_workspace_bytes(self, n_pairs, max_len):
        return int(lib().pgx_sw_workspace_bytes(self._h, int(n_pairs), int(max_len)))

    def sw_round_pairs(self, with_stats):
        """How many pairs one round of the score pass (with_stats false) or of the pass with statistics holds on this
        device; a longer list gives every lane group a further pair per round (for the tests)."""
        return int(lib().pgx_sw_round_pairs(self._h, 1 if with_stats else 0))

    def sw_last_stats_pairs(self):
        """How many pairs of the last sw_pairs / sw_pairs_dev call took the pass with statistics."""
        return int(lib().pgx_sw_last_stats_pairs(self._h))

    def sw_pairs_dev(self, d_residues1, d_offsets1, n1, d_residues2, d_offsets2, n2, d_pair_a, d_pair_b, n_pairs, d_min_score,
                     max_len, d_out, d_ws, ws_bytes, stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_sw_pairs_dev(self._h, d_residues1, d_offsets1, int(n1), d_residues2, d_offsets2, int(n2), d_pair_a,
                                     d_pair_b, int(n_pairs), d_min_score, int(max_len), d_out, d_ws, int(ws_bytes), stream))

    def genome_sets_diff(self, a_rows, a_genomes, b_rows, b_genomes, n_rows, n_genomes):
        """(a_only, b_only) uint32 [n_genomes]: per genome the rows of the COO set A that B lacks and the other way round;
        a coordinate given twice counts once (pgx.h: pgx_genome_sets_diff)."""
        a_rows, a_genomes = _coo_args(a_rows, a_genomes)
        b_rows, b_genomes = _coo_args(b_rows, b_genomes)
        a_only = np.zeros(int(n_genomes), dtype=np.uint32)
        b_only = np.zeros(int(n_genomes), dtype=np.uint32)
        check(lib().pgx_genome_sets_diff(self._h, _ptr(a_rows), _ptr(a_genomes), a_rows.size, _ptr(b_rows), _ptr(b_genomes),
                                         b_rows.size, int(n_rows), int(n_genomes), _ptr(a_only), _ptr(b_only)))
        return a_only, b_only

    def genome_sets_diff_dev(self, d_a_bits, d_b_bits, n_rows, n_genomes, d_a_only, d_b_only, stream=0):
        """The same on device bitmaps (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_genome_sets_diff_dev(self._h, d_a_bits, d_b_bits, int(n_rows), int(n_genomes), d_a_only, d_b_only,
                                             stream))

    # -- windows of a text, records grouped per gene (pangenome.build_proximal_pangenome) ------------------------------------
    def prox_cut(self, text, start, length, reverse):
        """(out, out_offsets, bad): window i -- the length[i] bytes of `text` (bytes or a 1-D uint8 array) at start[i],
        reverse-complemented where reverse[i] is set -- is out[out_offsets[i]:out_offsets[i + 1]]; bad[i] = 1 where a reverse
        window holds a byte without a complement, which comes out as 0 (pgx.h: pgx_prox_cut)."""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(text, dtype=np.uint8)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        start = np.ascontiguousarray(start, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        reverse = np.ascontiguousarray(reverse, dtype=np.uint8)
        if text.ndim != 1 or start.ndim != 1 or start.shape != length.shape or start.shape != reverse.shape:
            raise ValueError('text must be 1-D and start, length, reverse 1-D arrays of one length')
        out_offsets = np.zeros(start.size + 1, dtype=np.uint64)
        np.cumsum(length, dtype=np.uint64, out=out_offsets[1:])
        out = np.zeros(min(int(out_offsets[-1]), (1 << 32) - 1), dtype=np.uint8)     # (a larger one is refused)
        bad = np.zeros(start.size, dtype=np.uint8)
        check(lib().pgx_prox_cut(self._h, _ptr(text), text.size, _ptr(start), _ptr(length), _ptr(reverse), start.size,
                                 _ptr(out), _ptr(bad)))
        return out, out_offsets, bad

    def prox_cut_dev(self, d_text, text_bytes, d_start, d_length, d_reverse, d_out_offsets, n, d_out, d_bad, stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_prox_cut_dev(self._h, d_text, int(text_bytes), d_start, d_length, d_reverse, d_out_offsets, int(n),
                                     d_out, d_bad, stream))

    def prox_group(self, blob, offsets, gene, flags=0):
        """(first, variant, n_distinct) of the records blob[offsets[i]:offsets[i + 1]] keyed by gene[i]: the smallest
        index of an equal record, and the number of distinct records of the gene that appear before it (pgx.h:
        pgx_prox_group). flags: PROX_NARROW_HASH, the test seam."""
        blob, offsets = self._string_args(blob, offsets)
        gene = np.ascontiguousarray(gene, dtype=np.int32)
        if gene.ndim != 1 or gene.size != offsets.size - 1:
            raise ValueError('gene must hold one entry per record')
        first = np.zeros(gene.size, dtype=np.int32)
        variant = np.zeros(gene.size, dtype=np.int32)
        distinct = C.c_uint32(0)
        check(lib().pgx_prox_group(self._h, _ptr(blob), _ptr(offsets), _ptr(gene), gene.size, int(flags), _ptr(first),
                                   _ptr(variant), C.byref(distinct)))
        return first, variant, int(distinct.value)

    def prox_group_workspace_bytes(self, n):
        return int(lib().pgx_prox_group_workspace_bytes(int(n)))

    def prox_group_dev(self, d_blob, d_offsets, d_gene, n, d_first, d_variant, d_n_distinct, d_ws, ws_bytes, flags=0,
                       stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_prox_group_dev(self._h, d_blob, d_offsets, d_gene, int(n), int(flags), d_first, d_variant,
                                       d_n_distinct, d_ws, int(ws_bytes), stream))

    # -- rows of ids without repeats, runs of rows voted (pangenome.extract_annotations) -------------------------------------
    def annot_vote(self, tok, row_off, run_off, flags=0):
        """(keep uint8 [n_tokens], winner int32 [n_runs], votes uint32 [n_runs], differs uint8 [n_rows]) of the rows
        tok[row_off[r]:row_off[r + 1]] grouped into the runs [run_off[u], run_off[u + 1]): the first occurrences of a row's
        ids, the first row of each run's most frequent list of kept ids, how many rows hold that list, and the rows that hold
        another (pgx.h: pgx_annot_vote). flags: ANNOT_NARROW_HASH, the test seam."""
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        run_off = np.ascontiguousarray(run_off, dtype=np.uint32)
        if tok.ndim != 1 or row_off.ndim != 1 or run_off.ndim != 1 or row_off.size < 1 or run_off.size < 1:
            raise ValueError('tok must be 1-D, row_off hold n_rows + 1 and run_off n_runs + 1 entries')
        if int(row_off[-1]) > tok.size:
            raise ValueError('row_off runs past the end of tok')
        n_rows, n_runs = row_off.size - 1, run_off.size - 1
        keep = np.zeros(int(row_off[-1]), dtype=np.uint8)
        winner = np.zeros(n_runs, dtype=np.int32)
        votes = np.zeros(n_runs, dtype=np.uint32)
        differs = np.zeros(n_rows, dtype=np.uint8)
        check(lib().pgx_annot_vote(self._h, _ptr(tok), _ptr(row_off), n_rows, _ptr(run_off), n_runs, int(flags), _ptr(keep),
                                   _ptr(winner), _ptr(votes), _ptr(differs)))
        return keep, winner, votes, differs

    def annot_vote_workspace_bytes(self, n_rows, n_tokens, n_runs):
        return int(lib().pgx_annot_vote_workspace_bytes(int(n_rows), int(n_tokens), int(n_runs)))

    def annot_vote_dev(self, d_tok, d_row_off, n_rows, n_tokens, d_run_off, n_runs, d_keep, d_winner, d_votes, d_differs,
                       d_ws, ws_bytes, flags=0, stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_annot_vote_dev(self._h, d_tok, d_row_off, int(n_rows), int(n_tokens), d_run_off, int(n_runs),
                                       int(flags), d_keep, d_winner, d_votes, d_differs, d_ws, int(ws_bytes), stream))

    # -- path lengths in a directed graph, terms in strings (amr.build_resistome, generate_probable_hits_from_annotations) ---
    def graph_reach(self, succ_off, succ, targets, sources, return_rounds=False):
        """len uint32 [n_sources, n_targets]: the number of nodes on a shortest path from sources[s] to targets[t] of the
        graph whose node v has the successors succ[succ_off[v]:succ_off[v + 1]]; 1 for the node itself, 0 for no path
        (pgx.h: pgx_graph_reach). return_rounds: also the rounds the device ran."""
        succ_off = np.ascontiguousarray(succ_off, dtype=np.uint32)
        succ = np.ascontiguousarray(succ, dtype=np.uint32)
        targets = np.ascontiguousarray(targets, dtype=np.uint32)
        sources = np.ascontiguousarray(sources, dtype=np.uint32)
        if succ_off.ndim != 1 or succ.ndim != 1 or targets.ndim != 1 or sources.ndim != 1 or succ_off.size < 1:
            raise ValueError('succ_off must hold n_nodes + 1 entries; succ, targets and sources must be 1-D')
        if int(succ_off[-1]) > succ.size:
            raise ValueError('succ_off runs past the end of succ')
        out = np.zeros((sources.size, targets.size), dtype=np.uint32)
        rounds = C.c_uint32(0)
        check(lib().pgx_graph_reach(self._h, _ptr(succ_off), _ptr(succ), succ_off.size - 1, _ptr(targets), targets.size,
                                    _ptr(sources), sources.size, _ptr(out), C.byref(rounds)))
        return (out, int(rounds.value)) if return_rounds else out

    def graph_reach_workspace_bytes(self, n_nodes, n_targets, n_sources):
        return int(lib().pgx_graph_reach_workspace_bytes(int(n_nodes), int(n_targets), int(n_sources)))

    def graph_reach_dev(self, d_succ_off, d_succ, n_nodes, n_edges, d_targets, n_targets, d_sources, n_sources, d_out_len,
                        d_out_rounds, d_ws, ws_bytes, stream=0):
        """The same on device memory (raw device addresses, None for no rounds; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_graph_reach_dev(self._h, d_succ_off, d_succ, int(n_nodes), int(n_edges), d_targets, int(n_targets),
                                        d_sources, int(n_sources), d_out_len, d_out_rounds, d_ws, int(ws_bytes), stream))

    def term_scan(self, text, start, length, terms, term_off, flags=0):
        """mask uint64 [n, ceil(n_terms / 64)]: bit t & 63 of word t >> 6 of row i is set iff the term
        terms[term_off[t]:term_off[t + 1]] occurs in the length[i] bytes of `text` (bytes or a 1-D uint8 array) at start[i]
        (pgx.h: pgx_term_scan). flags: TERM_FOLD_ASCII compares A-Z as a-z."""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(text, dtype=np.uint8)
        if isinstance(terms, (bytes, bytearray, memoryview)):
            terms = np.frombuffer(terms, dtype=np.uint8)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        terms = np.ascontiguousarray(terms, dtype=np.uint8)
        start = np.ascontiguousarray(start, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        term_off = np.ascontiguousarray(term_off, dtype=np.uint32)
        if text.ndim != 1 or terms.ndim != 1 or start.ndim != 1 or start.shape != length.shape or term_off.ndim != 1 \
                or term_off.size < 1:
            raise ValueError('text, terms, start and length must be 1-D and term_off hold n_terms + 1 entries')
        if int(term_off[-1]) > terms.size:
            raise ValueError('term_off runs past the end of terms')
        n_terms = term_off.size - 1
        mask = np.zeros((start.size, (n_terms + 63) // 64), dtype=np.uint64)
        check(lib().pgx_term_scan(self._h, _ptr(text), text.size, _ptr(start), _ptr(length), start.size, _ptr(terms),
                                  _ptr(term_off), n_terms, int(flags), _ptr(mask)))
        return mask

    def term_scan_dev(self, d_text, text_bytes, d_start, d_length, n, d_terms, d_term_off, n_terms, term_bytes, d_out_mask,
                      flags=0, stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_term_scan_dev(self._h, d_text, int(text_bytes), d_start, d_length, int(n), d_terms, d_term_off,
                                      int(n_terms), int(term_bytes), int(flags), d_out_mask, stream))

    # -- equal integer tuples counted, SIR classes inferred from MICs (amr_inference) ------------------------------------------
    def tuple_group(self, cols, flags=0):
        """(first int32 [n], count uint32 [n], n_distinct) of the n records cols[:, i] of an int32 array [k, n]: the smallest
        index of an equal record, and at that index how many records equal it, 0 elsewhere (pgx.h: pgx_tuple_group).
        flags: TUPLE_NARROW_HASH, the test seam."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        if cols.ndim != 2:
            raise ValueError('cols must be [k, n]')
        k, n = cols.shape
        first = np.zeros(n, dtype=np.int32)
        count = np.zeros(n, dtype=np.uint32)
        distinct = C.c_uint32(0)
        check(lib().pgx_tuple_group(self._h, _ptr(cols), n, k, int(flags), _ptr(first), _ptr(count), C.byref(distinct)))
        return first, count, int(distinct.value)

    def tuple_group_workspace_bytes(self, n, k):
        return int(lib().pgx_tuple_group_workspace_bytes(int(n), int(k)))

    def tuple_group_dev(self, d_cols, n, k, d_first, d_count, d_n_distinct, d_ws, ws_bytes, flags=0, stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_tuple_group_dev(self._h, d_cols, int(n), int(k), int(flags), d_first, d_count, d_n_distinct, d_ws,
                                        int(ws_bytes), stream))

    def mic_infer(self, class_begin, sir, role, fl_begin, tk_begin, fvals, tvals, case, sign, combo, kind, token, value):
        """out int32 [n]: the sir code of the first class entry of case[i] that takes row i, -1 for none, -2 for a row the
        host has to decide (pgx.h: pgx_mic_infer, where every array is described)."""
        class_begin, fl_begin, tk_begin = (np.ascontiguousarray(a, dtype=np.uint32) for a in (class_begin, fl_begin, tk_begin))
        sir, tvals, case, token = (np.ascontiguousarray(a, dtype=np.int32) for a in (sir, tvals, case, token))
        role, sign, combo, kind = (np.ascontiguousarray(a, dtype=np.uint8) for a in (role, sign, combo, kind))
        fvals, value = (np.ascontiguousarray(a, dtype=np.float64) for a in (fvals, value))
        n_entries, n = sir.size, case.size
        if class_begin.ndim != 1 or class_begin.size < 1 or fl_begin.shape != (n_entries + 1,) or fl_begin.shape != tk_begin.shape \
                or role.shape != (n_entries,):
            raise ValueError('class_begin must hold n_cases + 1, fl_begin and tk_begin n_entries + 1 and role n_entries entries')
        if any(a.shape != (n,) for a in (sign, combo, kind, token, value)):
            raise ValueError('case, sign, combo, kind, token and value must hold one entry per row')
        out = np.zeros(n, dtype=np.int32)
        check(lib().pgx_mic_infer(self._h, _ptr(class_begin), class_begin.size - 1, _ptr(sir), _ptr(role), _ptr(fl_begin),
                                  _ptr(tk_begin), n_entries, _ptr(fvals), fvals.size, _ptr(tvals), tvals.size, _ptr(case),
                                  _ptr(sign), _ptr(combo), _ptr(kind), _ptr(token), _ptr(value), n, _ptr(out)))
        return out

    def mic_infer_dev(self, d_class_begin, n_cases, d_sir, d_role, d_fl_begin, d_tk_begin, n_entries, d_fvals, n_fvals, d_tvals,
                      n_tvals, d_case, d_sign, d_combo, d_kind, d_token, d_value, n, d_out, stream=0):
        """The same on device memory (raw device addresses; synchronises `stream`, see pgx.h)."""
        check(lib().pgx_mic_infer_dev(self._h, d_class_begin, int(n_cases), d_sir, d_role, d_fl_begin, d_tk_begin, int(n_entries),
                                      d_fvals, int(n_fvals), d_tvals, int(n_tvals), d_case, d_sign, d_combo, d_kind, d_token,
                                      d_value, int(n), d_out, stream))

    # -- the gene content of every node of a tree (weboflife.get_node_gene_content_table) ---------------------------------------
    def tree_content(self, rows, species, n_genes, n_species, leaf_species, child_off, child, order, level_off,
                     return_totals=False, counts=None):
        """(counts uint32 [n_nodes, tree_content_stride(n_genes)], duplicates), with return_totals (counts, totals uint32
        [n_nodes], duplicates): how many of the mapped nodes at or below each node carry each gene, and how many mapped nodes
        there are, for the 0/1 table whose ones are the records (rows[k], species[k]) and the tree pgx.h describes under
        pgx_tree_content. Pad entries of counts are zero. counts: a C-contiguous uint32 array of that shape to write into
        (a caller that asks chunk after chunk keeps one buffer, whose pages are then faulted in once)."""
        rows, species = _coo_args(rows, species)
        leaf_species = np.ascontiguousarray(leaf_species, dtype=np.int32)
        child_off, child, order, level_off = (np.ascontiguousarray(a, dtype=np.uint32) for a in (child_off, child, order, level_off))
        n_nodes = leaf_species.size
        if leaf_species.ndim != 1 or child_off.shape != (n_nodes + 1,) or order.shape != (n_nodes,) or child.ndim != 1 \
                or level_off.ndim != 1 or level_off.size < 1:
            raise ValueError('leaf_species and order must hold n_nodes, child_off n_nodes + 1 and level_off n_levels + 1 entries')
        if int(child_off[-1]) > child.size:
            raise ValueError('child_off runs past the end of child')
        shape = (n_nodes, self.tree_content_stride(n_genes))
        if counts is None:
            counts = np.zeros(shape, dtype=np.uint32)
        elif not (isinstance(counts, np.ndarray) and counts.dtype == np.uint32 and counts.shape == shape and counts.flags.c_contiguous
                  and counts.flags.writeable):
            raise ValueError('counts must be a writeable C-contiguous uint32 array of shape %r' % (shape,))
        totals = np.zeros(n_nodes, dtype=np.uint32) if return_totals else None
        dup = C.c_uint64(0)
        check(lib().pgx_tree_content(self._h, _ptr(rows), _ptr(species), rows.size, int(n_genes), int(n_species), _ptr(leaf_species),
                                     _ptr(child_off), _ptr(child), n_nodes, _ptr(order), _ptr(level_off), level_off.size - 1,
                                     _ptr(counts), _ptr(totals), C.byref(dup)))
        return (counts, totals, int(dup.value)) if return_totals else (counts, int(dup.value))

    @staticmethod
    def tree_content_stride(n_genes):
        return int(lib().pgx_tree_content_stride(int(n_genes)))

    def tree_content_workspace_bytes(self, n_nodes, n_genes, n_edges):
        return int(lib().pgx_tree_content_workspace_bytes(int(n_nodes), int(n_genes), int(n_edges)))

    def tree_content_dev(self, d_bits, n_genes, n_species, d_leaf_species, d_child_off, d_child, n_nodes, n_edges, d_order,
                         level_off, d_out_counts, d_out_totals, d_ws, ws_bytes, stream=0):
        """The same on device memory (raw device addresses, None for no totals); level_off alone is a host array: it sizes the
        launches. Only enqueues on `stream`, see pgx.h."""
        level_off = np.ascontiguousarray(level_off, dtype=np.uint32)
        if level_off.ndim != 1 or level_off.size < 1:
            raise ValueError('level_off must hold n_levels + 1 entries')
        check(lib().pgx_tree_content_dev(self._h, d_bits, int(n_genes), int(n_species), d_leaf_species, d_child_off, d_child,
                                         int(n_nodes), int(n_edges), d_order, _ptr(level_off), level_off.size - 1, d_out_counts,
                                         d_out_totals, d_ws, int(ws_bytes), stream))

    def pan_core(self, bits, n_genes, perms):
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        n_iter, n_genomes = perms.shape
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        stride = lib().pgx_bitmap_stride_words(int(n_genes))
        if bits.shape != (n_genomes, stride):
            raise ValueError('bitmap shape %r does not match (%d, %d)' % (bits.shape, n_genomes, stride))
        pan = np.empty((n_iter, n_genomes), dtype=np.int32)
        core = np.empty((n_iter, n_genomes), dtype=np.int32)
        check(lib().pgx_pan_core(self._h, _ptr(bits), int(n_genes), int(n_genomes), _ptr(perms),
                                 int(n_iter), _ptr(pan), _ptr(core)))
        return pan, core

    # -- K1/K2 ---------------------------------------------------------------
    def cluster_greedy(self, residues, offsets, params, want_stats=True):
        """want_stats=False: no work counters (stats is None in the result) and the library leaves out the look-ups
        that only the counters need (pgx.h); the clustering is the same."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out_cluster = np.empty(n, dtype=np.int32)
        out_member = np.empty(n, dtype=np.int32)
        out_identity = np.empty(n, dtype=np.float32)
        out_strand = np.zeros(n, dtype=np.uint8)
        n_clusters = C.c_uint32(0)
        stats = ClusterStats()
        check(lib().pgx_cluster_greedy(self._h, _ptr(residues), _ptr(offsets), n, C.byref(params),
                                       _ptr(out_cluster), _ptr(out_member), _ptr(out_identity),
                                       _ptr(out_strand), C.byref(n_clusters), C.byref(stats) if want_stats else None))
        return out_cluster, out_member, out_identity, out_strand, int(n_clusters.value), stats.as_dict() if want_stats else None


    def cluster_greedy_dev(self, d_residues, d_offsets, n, total_bytes, params, stream=0, want_stats=True):
        """Sequences resident in HBM (raw device addresses); outputs are host arrays."""
        out_cluster = np.empty(n, dtype=np.int32)
        out_member = np.empty(n, dtype=np.int32)
        out_identity = np.empty(n, dtype=np.float32)
        out_strand = np.zeros(n, dtype=np.uint8)
        n_clusters = C.c_uint32(0)
        stats = ClusterStats()
        check(lib().pgx_cluster_greedy_dev(self._h, d_residues, d_offsets, int(n), int(total_bytes),
                                           C.byref(params), _ptr(out_cluster), _ptr(out_member),
                                           _ptr(out_identity), _ptr(out_strand), C.byref(n_clusters),
                                           C.byref(stats) if want_stats else None, stream))
        return out_cluster, out_member, out_identity, out_strand, int(n_clusters.value), stats.as_dict() if want_stats else None


class FastaSet(object):
    """Genome FASTA files parsed, hashed and de-duplicated by libpgx's host side (csrc/ingest.cpp):
    what consolidate_seqs() (reference pangenome.py:336-405) computes, as arrays. `simple` is False
    when the files hold something the reference's line-by-line semantics treat specially (see
    pgx.h); the arrays are then unavailable and the caller takes the Python path."""

    def __init__(self, paths, threads=0):
        self._h = C.c_void_p()
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        check(lib().pgx_fasta_open(arr, len(paths), int(threads), C.byref(self._h)))
        info = FastaInfo()
        check(lib().pgx_fasta_info(self._h, C.byref(info)))
        self.n_records, self.n_missing, self.n_groups = int(info.n_records), int(info.n_missing), int(info.n_groups)
        self.simple, self.why = bool(info.simple), info.why.decode('utf-8', 'replace')
        self._n_res, self._n_hdr = int(info.n_residue_bytes), int(info.n_header_bytes)

    def close(self):
        h, self._h = self._h, C.c_void_p()      # (taken first: a second caller, e.g. __del__ on another thread, finds nothing)
        if h:
            lib().pgx_fasta_close(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _view(self, fn, dtype, n):
        """numpy view (no copy) of one of the library's arrays; valid until close()."""
        ptr = getattr(lib(), fn)(self._h)
        if not ptr or n == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=n)

    group_of_record = property(lambda self: self._view('pgx_fasta_group_of_record', np.int32, self.n_records))
    file_of_record = property(lambda self: self._view('pgx_fasta_file_of_record', np.uint32, self.n_records))
    rep_of_group = property(lambda self: self._view('pgx_fasta_rep_of_group', np.uint64, self.n_groups))
    residues = property(lambda self: self._view('pgx_fasta_residues', np.uint8, self._n_res))
    offsets = property(lambda self: self._view('pgx_fasta_offsets', np.uint64, self.n_groups + 1))
    letters = property(lambda self: self._view('pgx_fasta_letters', np.uint32, self.n_groups))
    digests = property(lambda self: self._view('pgx_fasta_digests', np.uint8, self.n_groups * 32))
    header_offsets = property(lambda self: self._view('pgx_fasta_header_offsets', np.uint64, self.n_records + 1))

    def headers(self, records=None):
        """Header strings of all records (or of the given record indices)."""
        blob = bytes(self._view('pgx_fasta_header_blob', np.uint8, self._n_hdr))
        off = self.header_offsets
        idx = range(self.n_records) if records is None else records
        return [blob[off[i]:off[i + 1]].decode('ascii') for i in idx]

    def write_consolidated(self, nr_path, shared_path, missing_path=None):
        check(lib().pgx_fasta_write_consolidated(self._h, os.fsencode(nr_path) if nr_path else None, os.fsencode(shared_path),
                                                 os.fsencode(missing_path) if missing_path else None))

    def feature_coo(self, cluster, member, file_order, genome_of_file):
        """Coordinates of the allele and the gene table (pgx_fasta_feature_coo). Returns a dict: allele_groups,
        gene_of_allele, n_genes, a_row, a_col, g_row, g_col, lost_records."""
        cluster = np.ascontiguousarray(cluster, dtype=np.int32)
        member = np.ascontiguousarray(member, dtype=np.int32)
        file_order = np.ascontiguousarray(file_order, dtype=np.int32)
        genome_of_file = np.ascontiguousarray(genome_of_file, dtype=np.int32)
        if not (cluster.size == member.size == self.n_groups) or file_order.size != genome_of_file.size:
            raise ValueError('one entry per non-redundant sequence / per file expected')
        groups = np.empty(self.n_groups, dtype=np.int64)
        gene_of = np.empty(self.n_groups, dtype=np.int32)
        coo = [np.empty(self.n_records, dtype=np.int32) for _ in range(4)]
        lost = np.empty(self.n_records, dtype=np.int64)
        n = [C.c_uint64(0) for _ in range(5)]    # alleles, genes, allele triples, gene triples, lost records
        check(lib().pgx_fasta_feature_coo(self._h, _ptr(cluster), _ptr(member), _ptr(file_order), _ptr(genome_of_file),
                                          _ptr(groups), _ptr(gene_of), C.byref(n[0]), C.byref(n[1]), _ptr(coo[0]), _ptr(coo[1]),
                                          C.byref(n[2]), _ptr(coo[2]), _ptr(coo[3]), C.byref(n[3]), _ptr(lost), C.byref(n[4])))
        na, ng, ta, tg, nl = (int(x.value) for x in n)
        return {'allele_groups': groups[:na], 'gene_of_allele': gene_of[:na], 'n_genes': ng, 'a_row': coo[0][:ta],
                'a_col': coo[1][:ta], 'g_row': coo[2][:tg], 'g_col': coo[3][:tg], 'lost_records': lost[:nl]}

    def write_clustered(self, cluster, member, identity, strand, nucleotide, prefix, variant,
                        clstr_path=None, names_path=None, nr_out_path=None):
        cluster = np.ascontiguousarray(cluster, dtype=np.int32)
        member = np.ascontiguousarray(member, dtype=np.int32)
        identity = np.ascontiguousarray(identity, dtype=np.float32)
        strand = None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)
        if not (cluster.size == member.size == identity.size == self.n_groups):
            raise ValueError('one entry per non-redundant sequence expected')
        enc = lambda x: os.fsencode(x) if x else None   # noqa: E731
        check(lib().pgx_fasta_write_clustered(self._h, _ptr(cluster), _ptr(member), _ptr(identity), _ptr(strand),
                                              1 if nucleotide else 0, prefix.encode(), variant.encode(),
                                              enc(clstr_path), enc(names_path), enc(nr_out_path)))


def format_labels(prefix, cluster, member=None, variant=None):
    """numpy unicode array of feature names <prefix><cluster>[<variant><member>] (reference
    pangenome.py:1944-1969), formatted by the library."""
    cluster = np.ascontiguousarray(cluster, dtype=np.int32)
    if variant is not None:
        member = np.ascontiguousarray(member, dtype=np.int32)
    digits = lambda a: len(str(int(a.max()))) if a.size else 1   # noqa: E731
    if prefix.isascii() and (variant is None or variant.isascii()) and (cluster.size == 0 or int(cluster.min()) >= 0) \
            and (variant is None or member.size == 0 or int(member.min()) >= 0):
        # straight into numpy's own 'U' layout (UCS-4), exact width, several threads
        width = len(prefix) + digits(cluster) + (len(variant) + digits(member) if variant is not None else 0)
        if width <= 64:
            out = np.zeros(cluster.size, dtype='U%d' % width)
            check(lib().pgx_format_labels_ucs4(prefix.encode(), variant.encode() if variant is not None else None,
                                               _ptr(cluster), _ptr(member) if variant is not None else None,
                                               cluster.size, width, _ptr(out)))
            return out
    width = len(prefix.encode()) + 11 + (len(variant) + 11 if variant is not None else 0)
    out = np.zeros(cluster.size, dtype='S%d' % width)
    check(lib().pgx_format_labels(prefix.encode(), variant.encode() if variant is not None else None, _ptr(cluster),
                                  _ptr(member) if variant is not None else None, cluster.size, width, _ptr(out)))
    return np.char.decode(out, 'utf-8')


def allele_order(cluster, member):
    """Positions of the (cluster, member) pairs in the order of their allele names sorted as strings (stable)."""
    cluster = np.ascontiguousarray(cluster, dtype=np.int32)
    member = np.ascontiguousarray(member, dtype=np.int32)
    if cluster.shape != member.shape or cluster.ndim != 1:
        raise ValueError('cluster and member must be 1-D arrays of one length')
    out = np.empty(cluster.size, dtype=np.int64)
    check(lib().pgx_allele_order(_ptr(cluster), _ptr(member), cluster.size, _ptr(out)))
    return out


def first_insertions(rows, cols, n_cols):
    """Ascending positions i at which the pair (rows[i], cols[i]) occurs for the first time."""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    if rows.shape != cols.shape or rows.ndim != 1:
        raise ValueError('rows and cols must be 1-D arrays of one length')
    out = np.empty(rows.size, dtype=np.int64)
    m = C.c_uint64(0)
    check(lib().pgx_first_insertions(_ptr(rows), _ptr(cols), rows.size, int(max(n_cols, 1)), _ptr(out), C.byref(m)))
    return out[:m.value]


_default_ctx = None


def default_context():
    """Process-wide context on device LOCAL_RANK (one process per GPU) or 0."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get('LOCAL_RANK', '0')))
    return _default_ctx
