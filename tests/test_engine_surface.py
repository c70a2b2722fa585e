"""The Python engines keep their public surface: every public name of CosineEngine and NodeEngine with its signature
(inspect.signature), recorded from the commit before their shared request-family methods moved into one base class."""
import inspect

RECORDED = {'CosineEngine': {'batched_last_counters': "(self) -> 'dict'",
                  'batched_pass2_pairs': "(self) -> 'dict'",
                  'bound_enqueue_row_keys_streamed': "(self, topn: 'int', stream=None)",
                  'bound_query_row_topn': "(self, topn: 'int')",
                  'bucket_sample_info': "(self) -> 'dict'",
                  'bucket_sample_rows': '(self)',
                  'close': "(self) -> 'None'",
                  'debug_handoff': "(self, flags: 'int') -> 'None'",
                  'enqueue_batch_keys': "(self, queries, exclude_global, topn: 'int', out_keys, stream=None) -> 'None'",
                  'enqueue_batch_keys_dev': "(self, queries_dev, exclude_dev, topn: 'int', out_keys, stream=None) -> 'None'",
                  'enqueue_batch_keys_streamed': "(self, queries, exclude_global, topn: 'int', out_keys, stream=None) -> 'None'",
                  'enqueue_flush': "(self, stream=None) -> 'None'",
                  'enqueue_merge_keys': "(self, lists, n_lists: 'int', list_len: 'int', topn: 'int', out_keys, out_idx=None, out_score=None, "
                                        "stream=None) -> 'None'",
                  'enqueue_merge_keys_batch': "(self, lists, n_lists: 'int', list_len: 'int', list_stride: 'int', query_stride: 'int', batch: 'int', "
                                              "topn: 'int', out_keys, out_idx=None, out_score=None, stream=None) -> 'None'",
                  'enqueue_query_keys': "(self, query, exclude_global: 'int', topn: 'int', out_keys, stream=None) -> 'None'",
                  'enqueue_query_keys_streamed': "(self, query, exclude_global: 'int', topn: 'int', out_keys, stream=None) -> 'None'",
                  'enqueue_row_keys': "(self, local_row: 'int', topn: 'int', out_keys, stream=None) -> 'None'",
                  'enqueue_row_keys_streamed': "(self, local_row: 'int', topn: 'int', out_keys, stream=None) -> 'None'",
                  'enqueue_scores': "(self, local_row: 'int', query, out_scores, stream=None) -> 'None'",
                  'enqueue_stream_probe': "(self, sink, stream=None, which: 'int' = 0) -> 'None'",
                  'fetch_rows': "(self, local_rows) -> 'np.ndarray'",
                  'label_counters': "(self) -> 'dict'",
                  'lane': '(self) -> "\'CosineEngine\'"',
                  'lane_status': "(self) -> 'dict'",
                  'own_stream': '(self)',
                  'playlist_counters': "(self) -> 'dict'",
                  'query_batch_topn': "(self, queries, exclude_global, topn: 'int')",
                  'query_mean_topn': "(self, queries, topn: 'int', exclude=None, where=None, weights=None, labels=None, prior_weight=None, "
                                     "scales=None, seen=None, only=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                  'query_mean_topn_capped': "(self, queries, topn: 'int', max_per_group: 'int', lam=1.0, pool=None, exclude=None, where=None, "
                                            'weights=None, return_mmr=False, return_pool_rows=False, labels=None, prior_weight=None, seen=None, '
                                            'only=None)',
                  'query_mean_topn_diverse': "(self, queries, topn: 'int', lam, pool=None, exclude=None, where=None, weights=None, return_mmr=False, "
                                             'labels=None, prior_weight=None, seen=None, only=None)',
                  'query_nearest': "(self, members, topn: 'int', exclude=None, where=None, labels=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                  'query_nearest_rows': "(self, rows, topn: 'int', exclude=None, where=None, labels=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                  'query_nearest_rows_scaled': "(self, rows, topn: 'int', scales, exclude=None, where=None, labels=None, seen=None, only=None) -> "
                                               "'Tuple[np.ndarray, np.ndarray]'",
                  'query_nearest_scaled': "(self, members, topn: 'int', scales, exclude=None, where=None, labels=None, seen=None, only=None) -> "
                                          "'Tuple[np.ndarray, np.ndarray]'",
                  'query_playlist_topn': "(self, local_rows, topn: 'int', exclude=None, where=None, weights=None, labels=None, prior_weight=None, "
                                         "scales=None, seen=None, only=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                  'query_playlist_topn_capped': "(self, local_rows, topn: 'int', max_per_group: 'int', lam=1.0, pool=None, exclude=None, where=None, "
                                                'weights=None, return_mmr=False, return_pool_rows=False, labels=None, prior_weight=None, seen=None, '
                                                'only=None)',
                  'query_playlist_topn_diverse': "(self, local_rows, topn: 'int', lam, pool=None, exclude=None, where=None, weights=None, "
                                                 'return_mmr=False, labels=None, prior_weight=None, seen=None, only=None)',
                  'query_row_topn': "(self, local_row: 'int', topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                  'query_row_topn_labels': "(self, local_row: 'int', labels, topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                  'query_topn': "(self, query, exclude_global: 'int', topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                  'query_topn_labels': "(self, query, exclude_global: 'int', labels, topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                  'rebuild_replica': "(self) -> 'None'",
                  'replica_counters': "(self) -> 'dict'",
                  'replica_entries': '(self, local_rows)',
                  'row_set': "(self, ids) -> 'RowSet'",
                  'scores': "(self, query) -> 'np.ndarray'",
                  'scores_row': "(self, local_row: 'int') -> 'np.ndarray'",
                  'set_batch_path': "(self, path: 'int') -> 'None'",
                  'set_groups': "(self, groups) -> 'None'",
                  'set_labels': "(self, labels) -> 'None'",
                  'set_priors': "(self, priors) -> 'None'",
                  'set_replica': "(self, mode: 'int') -> 'None'",
                  'set_sample': "(self, mode: 'int') -> 'None'",
                  'set_timing': "(self, enabled) -> 'None'",
                  'stats': "(self) -> 'capi.Stats'",
                  'update_info': "(self) -> 'dict'",
                  'update_rows': "(self, local_rows, feats=None) -> 'None'"},
 'NodeEngine': {'close': "(self) -> 'None'",
                'enqueue_flush': "(self) -> 'None'",
                'enqueue_query': "(self, query, exclude_global: 'int', topn: 'int') -> 'int'",
                'enqueue_row': "(self, global_row: 'int', topn: 'int') -> 'int'",
                'info': "(self) -> 'dict'",
                'note': "(self) -> 'str'",
                'placement': "(self) -> 'int'",
                'query_batch_topn': "(self, queries, exclude_global, topn: 'int')",
                'query_mean_topn': "(self, queries, topn: 'int', exclude=None, where=None, weights=None, labels=None, prior_weight=None, "
                                   "scales=None, seen=None, only=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                'query_mean_topn_capped': "(self, queries, topn: 'int', max_per_group: 'int', lam=1.0, pool=None, exclude=None, where=None, "
                                          'weights=None, return_mmr=False, return_pool_rows=False, labels=None, prior_weight=None, seen=None, '
                                          'only=None)',
                'query_mean_topn_diverse': "(self, queries, topn: 'int', lam, pool=None, exclude=None, where=None, weights=None, return_mmr=False, "
                                           'labels=None, prior_weight=None, seen=None, only=None)',
                'query_nearest': "(self, members, topn: 'int', exclude=None, where=None, labels=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                'query_nearest_rows': "(self, rows, topn: 'int', exclude=None, where=None, labels=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                'query_nearest_rows_scaled': "(self, rows, topn: 'int', scales, exclude=None, where=None, labels=None, seen=None, only=None) -> "
                                             "'Tuple[np.ndarray, np.ndarray]'",
                'query_nearest_scaled': "(self, members, topn: 'int', scales, exclude=None, where=None, labels=None, seen=None, only=None) -> "
                                        "'Tuple[np.ndarray, np.ndarray]'",
                'query_playlist_topn': "(self, global_rows, topn: 'int', exclude=None, where=None, weights=None, labels=None, prior_weight=None, "
                                       "scales=None, seen=None, only=None) -> 'Tuple[np.ndarray, np.ndarray]'",
                'query_playlist_topn_capped': "(self, global_rows, topn: 'int', max_per_group: 'int', lam=1.0, pool=None, exclude=None, where=None, "
                                              'weights=None, return_mmr=False, return_pool_rows=False, labels=None, prior_weight=None, seen=None, '
                                              'only=None)',
                'query_playlist_topn_diverse': "(self, global_rows, topn: 'int', lam, pool=None, exclude=None, where=None, weights=None, "
                                               'return_mmr=False, labels=None, prior_weight=None, seen=None, only=None)',
                'query_row_topn': "(self, global_row: 'int', topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                'query_row_topn_labels': "(self, global_row: 'int', labels, topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                'query_topn': "(self, query, exclude_global: 'int', topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                'query_topn_labels': "(self, query, exclude_global: 'int', labels, topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'",
                'rccl_ranks': "(self) -> 'dict'",
                'row_set': "(self, ids) -> 'RowSet'",
                'rows_by_pointer': "(self) -> 'bool'",
                'scores_row': "(self, global_row: 'int') -> 'np.ndarray'",
                'set_groups': "(self, groups) -> 'None'",
                'set_labels': "(self, labels) -> 'None'",
                'set_priors': "(self, priors) -> 'None'",
                'set_replica': "(self, mode: 'int') -> 'None'",
                'set_timing': "(self, enabled) -> 'None'",
                'set_transport': "(self, transport: 'int') -> 'None'",
                'set_window': "(self, window: 'int') -> 'None'",
                'set_window_mode': "(self, batched: 'bool') -> 'None'",
                'shard_stats': "(self, shard: 'int') -> 'capi.Stats'",
                'stream_stats': "(self) -> 'dict'",
                'update_rows': "(self, global_rows, feats) -> 'None'",
                'wait': "(self, ticket: 'int', topn: 'int') -> 'Tuple[np.ndarray, np.ndarray]'"}}


def _surface(cls):
    out = {}
    for name in (n for n in dir(cls) if not n.startswith("_")):
        member = getattr(cls, name)
        out[name] = str(inspect.signature(member)) if callable(member) else "attribute"
    return out


def test_public_names_and_signatures_are_the_recorded_ones():
    from spotify_recommender_amd.engine import CosineEngine, NodeEngine
    for cls in (CosineEngine, NodeEngine):
        assert _surface(cls) == RECORDED[cls.__name__], cls.__name__


def test_the_shared_methods_are_defined_once():
    from spotify_recommender_amd.engine import CosineEngine, NodeEngine
    for name in ("query_mean_topn", "query_nearest", "query_nearest_rows", "query_nearest_scaled", "query_nearest_rows_scaled",
                 "query_mean_topn_diverse", "query_mean_topn_capped", "set_labels", "set_groups", "set_priors", "_playlist", "_nearest"):
        assert getattr(CosineEngine, name) is getattr(NodeEngine, name), name
