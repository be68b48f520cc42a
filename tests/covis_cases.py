"""Shared by the covisibility tests: ctypes wrappers of the serial host build (csrc/host/covis_host.cpp over csrc/covis_spec.h), a
restatement of steps 1 - 5 of the rule in plain Python (sets and a breadth-first search), the graphs of the rule tests and the two-place
scene of the localisation tests."""
import ctypes
from collections import deque

import numpy as np

import triangulate_cases as TC

CV_MAX_LIST, W = 1024, 8
_host = None


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        h = ctypes.CDLL(build.build_covis_host(verbose=False))      # (stamp-guarded: rebuilt only after an edit of the rule's text)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        h.gf_covis_host_lists.restype, h.gf_covis_host_lists.argtypes = ci, [vp, vp, ci, vp, ci, vp, vp, ci] + [vp] * 7
        h.gf_covis_host_cluster.restype, h.gf_covis_host_cluster.argtypes = ci, [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp, vp]
        h.gf_covis_host_rows.restype = ci
        h.gf_covis_host_rows.argtypes = [vp, vp, ci, ci, vp, ci, vp, ci, vp, ci, ci, vp, vp, ci, vp, ci, ci, ci] + [vp] * 9
        h.gf_covis_host_select.restype = None
        h.gf_covis_host_select.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, ci, ci] + [vp] * 8
        _host = h
    return _host


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pad(a):
    """ctypes wants an address: an empty array is passed as one spare element"""
    return a if a.size else np.zeros(1, a.dtype)


# --------------------------------------------------------------------------------------------- cases
def make_case(n_images, queries, tracks, pairs, seed=0, extra=1, query_kp=4):
    """queries: image indices in query order.  tracks: per point the (distinct) images that observe it.  pairs: (i, j, rows) with rows either
    a number of random rows or a list of (keypoint of i, keypoint of j).  A database image's keypoints are its observations in point order,
    then `extra` keypoints without a point; a query has query_kp keypoints and no point."""
    rng = np.random.default_rng(seed)
    per_image = [[] for _ in range(n_images)]
    obs_off, obs_img = [0], []
    for t, imgs in enumerate(tracks):
        for i in sorted(int(v) for v in imgs):
            per_image[i].append(t)
            obs_img.append(i)
        obs_off.append(len(obs_img))
    image_q = np.full(n_images, -1, np.int32)
    image_q[list(queries)] = np.arange(len(queries))
    assert all(not per_image[q] for q in queries)
    counts = [query_kp if image_q[i] >= 0 else len(per_image[i]) + extra for i in range(n_images)]
    kp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pok = np.full(int(kp_off[-1]), -1, np.int32)
    for i in range(n_images):
        pok[kp_off[i]:kp_off[i] + len(per_image[i])] = per_image[i]
    pim, id_off, ids = [], [0], []
    for i, j, rows in pairs:
        if isinstance(rows, (int, np.integer)):
            rows = [(int(rng.integers(counts[i])), int(rng.integers(counts[j]))) for _ in range(rows)] if counts[i] and counts[j] else []
        pim.append((i, j)), ids.extend(rows), id_off.append(len(ids))
    return {'n_images': n_images, 'Q': len(queries), 'T': len(tracks), 'image_q': image_q, 'kp_off': kp_off, 'pok': pok,
            'obs_offsets': np.array(obs_off, np.int32), 'obs_image': np.array(obs_img, np.int32), 'pair_images': np.array(pim, np.int32).reshape(-1, 2),
            'id_off': np.array(id_off, np.int32), 'ids': np.array(ids, np.int32).reshape(-1, 2)}


def chain_case(L):
    """one query (image 0) and L database images 1 .. L in one chain: point k is seen by images k + 1 and k + 2; the pairs name the far end
    first, one row each"""
    return make_case(L + 1, [0], [(k + 1, k + 2) for k in range(L - 1)], [(0, i, [(0, 0)]) for i in range(L, 0, -1)], extra=0)


def random_case(seed):
    rng = np.random.default_rng(seed)
    Q, n_db = int(rng.integers(1, 7)), int(rng.integers(1, 41))
    n = Q + n_db
    queries = sorted(rng.choice(n, Q, replace=False).tolist())
    db = [i for i in range(n) if i not in queries]
    tracks = [rng.choice(db, min(int(rng.integers(2, 9)), n_db), replace=False).tolist() for _ in range(int(rng.integers(0, 201)))]
    pairs = []
    for q in queries:
        for d in rng.choice(db, int(rng.integers(1, n_db + 1)), replace=False).tolist():
            pairs.append((q, d, int(rng.integers(0, 12))) if rng.random() < 0.5 else (d, q, int(rng.integers(0, 12))))
    for _ in range(int(rng.integers(0, 4))):                            # pairs that contribute nothing: database - database, query - query
        pairs.append((db[0], db[-1], 3))
        pairs.append((queries[0], queries[-1], 2))
    rng.shuffle(pairs)
    return make_case(n, queries, tracks, [tuple(p) for p in pairs], seed=seed, extra=int(rng.integers(0, 3)))


def rule_cases():
    """name -> case: the cases of the rule tests (the list of 1025 is chain_case(1025), which only the error tests build)"""
    c = {
        'no_pairs': make_case(3, [0], [(1, 2)], []),
        'one_database_image': make_case(3, [0], [(1, 2)], [(0, 1, 5)]),
        'two_images_no_shared_point': make_case(5, [0], [(1, 3), (2, 4)], [(0, 1, 4), (0, 2, 4)]),
        # a - b - c linked only through b: a = 1, b = 2, c = 3
        'bridge_outside_the_list': make_case(4, [0], [(1, 2), (2, 3)], [(0, 1, 4), (0, 3, 4)]),
        'bridge_inside_the_list': make_case(4, [0], [(1, 2), (2, 3)], [(0, 1, 4), (0, 3, 4), (0, 2, 4)]),
        'star': make_case(8, [0], [(4, k) for k in (1, 2, 3, 5, 6, 7)], [(0, k, 3) for k in range(1, 8)]),
        'image_without_points': make_case(4, [0], [(1, 2)], [(0, 3, 4), (0, 1, 4), (0, 2, 4)]),
        'query_on_the_second_side': make_case(4, [3], [(0, 1), (1, 2)], [(0, 3, 4), (3, 1, 4), (2, 3, 4)]),
        'pair_listed_twice': make_case(3, [0], [(1, 2)], [(0, 1, 5), (0, 2, 3), (0, 1, 5)]),
        # keypoints 0 and 1 of images 1 and 2 hold points 0 and 1, keypoint 2 none: (query keypoint 2, point 0) occurs three times
        'repeated_rows': make_case(3, [0], [(1, 2), (1, 2)], [(0, 1, [(2, 0), (2, 1), (2, 0), (3, 2)]), (2, 0, [(0, 2), (2, 2), (2, 1)])]),
        'two_queries_share_images': make_case(6, [0, 5], [(1, 2), (3, 4)], [(0, 1, 4), (5, 3, 4), (0, 3, 4), (2, 5, 4), (0, 4, 2), (5, 1, 3)]),
        'chain_1024': chain_case(1024),
    }
    for s in range(30):
        c[f'random_{s:02d}'] = random_case(1000 + s)
    return c


# --------------------------------------------------------------------------------------------- the rule in plain Python
def python_rule(c, cluster=True, dedup=False):
    """Steps 1 - 5 of csrc/covis_spec.h with sets and a breadth-first search -> the tables and per-row outputs the host build writes."""
    n, Q = c['n_images'], c['Q']
    has_pts = [bool((c['pok'][c['kp_off'][i]:c['kp_off'][i + 1]] >= 0).any()) for i in range(n)]
    lists, pairs = [[] for _ in range(Q)], []
    for p, (i, j) in enumerate(c['pair_images'].tolist()):
        for qs, ds, col in ((i, j, 0), (j, i, 1)):
            if c['image_q'][qs] >= 0 and c['image_q'][ds] < 0 and has_pts[ds]:
                q = int(c['image_q'][qs])
                if ds not in lists[q]:
                    lists[q].append(ds)
                pairs.append((q, qs, ds, int(c['id_off'][p]), int(c['id_off'][p + 1]), col, lists[q].index(ds), 0))
                break
    if any(len(x) > CV_MAX_LIST for x in lists):
        return None
    seen_by = [set(c['obs_image'][c['obs_offsets'][t]:c['obs_offsets'][t + 1]].tolist()) for t in range(c['T'])]
    points_of = [set() for _ in range(n)]
    for t, s in enumerate(seen_by):
        for i in s:
            points_of[i].add(t)
    cluster_of, n_clusters = [], []
    for q in range(Q):
        L = len(lists[q])
        label = [-1] * L
        count = 0
        for a in range(L):                                              # ascending: a new component is found at its smallest position
            if label[a] >= 0 or not cluster:
                continue
            label[a] = count
            todo = deque([a])
            while todo:
                x = todo.popleft()
                for b in range(L):
                    if label[b] < 0 and points_of[lists[q][x]] & points_of[lists[q][b]]:
                        label[b] = count
                        todo.append(b)
            count += 1
        if not cluster:
            label, count = [0] * L, int(L > 0)
        cluster_of.append(label), n_clusters.append(count)
    prob_base = np.concatenate([[0], np.cumsum(n_clusters)]).astype(np.int32)
    rows = []                                                           # (original row, query node, point, problem, keep)
    for q, qs, ds, rb, re, col, pos, _ in pairs:
        for e in range(rb, re):
            kq, kd = int(c['ids'][e][col]), int(c['ids'][e][1 - col])
            pt = int(c['pok'][c['kp_off'][ds] + kd])
            rows.append((len(rows), int(c['kp_off'][qs]) + kq, pt, int(prob_base[q]) + cluster_of[q][pos], int(pt >= 0)))
    M0, N = len(rows), int(prob_base[-1])
    first_of, slot, sel, prob_off = np.full(M0, -1, np.int32), np.full(M0, -1, np.int32), [], [0]
    for k in range(N):
        seen = {}
        for r, node, pt, prob, keep in rows:
            if prob != k or not keep:
                continue
            first = seen.setdefault((node, pt), r) if dedup else r
            first_of[r] = first
            if first == r:
                slot[r] = len(sel)
                sel.append(r)
            else:
                slot[r] = slot[first]
        prob_off.append(len(sel))
    flat = lambda xs: np.array([v for x in xs for v in x], np.int32)    # noqa: E731
    by_id = [sorted(range(len(x)), key=x.__getitem__) for x in lists]
    return {'pairs': np.array(pairs, np.int32).reshape(-1, W),
            'pair_row_off': np.concatenate([[0], np.cumsum([p[4] - p[3] for p in pairs])]).astype(np.int32),
            'list_off': np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32), 'list_img': flat(lists),
            'sorted_img': flat([[x[a] for a in o] for x, o in zip(lists, by_id)]), 'sorted_pos': flat(by_id),
            'cluster': flat(cluster_of), 'n_clusters': np.array(n_clusters, np.int32).reshape(-1), 'prob_base': prob_base,
            'row_kp': np.array([r[1] for r in rows], np.int32), 'row_pt': np.array([r[2] if r[4] else -1 for r in rows], np.int32),
            'row_prob': np.array([r[3] for r in rows], np.int32), 'keep': np.array([r[4] for r in rows], np.uint8),
            'first_of': first_of, 'slot': slot, 'sel': np.array(sel, np.int32), 'prob_off': np.array(prob_off, np.int32)}


# --------------------------------------------------------------------------------------------- the host build
TABLE_KEYS = ('pairs', 'pair_row_off', 'list_off', 'list_img', 'sorted_img', 'sorted_pos')
ROW_KEYS = ('row_kp', 'row_pt', 'row_prob', 'keep', 'first_of', 'slot', 'sel', 'prob_off')


def host_lists(c):
    """-> (rc, tables dict) of step 1"""
    P, Q = len(c['pair_images']), c['Q']
    pairs, pro = np.zeros((P + 1, W), np.int32), np.zeros(P + 1, np.int32)
    loff, limg, simg, spos = np.zeros(Q + 1, np.int32), *(np.zeros(P + 1, np.int32) for _ in range(3))
    sizes = np.zeros(3, np.int32)
    rc = host_lib().gf_covis_host_lists(_p(_pad(c['pair_images'])), _p(c['id_off']), P, _p(c['image_q']), c['n_images'], _p(c['kp_off']),
                                        _p(_pad(c['pok'])), Q, _p(pairs), _p(pro), _p(loff), _p(limg), _p(simg), _p(spos), _p(sizes))
    C, _, Lt = (int(v) for v in sizes)
    return rc, {'pairs': pairs[:C].copy(), 'pair_row_off': pro[:C + 1].copy(), 'list_off': loff, 'list_img': limg[:Lt].copy(),
                'sorted_img': simg[:Lt].copy(), 'sorted_pos': spos[:Lt].copy()}


def host_cluster(c, tb, enable=True):
    """-> (status, cluster [L], n_clusters [Q]) of steps 2 and 3"""
    Lt, Q = len(tb['list_img']), c['Q']
    cluster, ncl = np.zeros(max(Lt, 1), np.int32), np.zeros(max(Q, 1), np.int32)
    st = host_lib().gf_covis_host_cluster(_p(c['kp_off']), c['n_images'], _p(_pad(c['pok'])), len(c['pok']), _p(c['obs_offsets']), c['T'],
                                          _p(_pad(c['obs_image'])), len(c['obs_image']), _p(tb['list_off']), _p(_pad(tb['list_img'])),
                                          _p(_pad(tb['sorted_img'])), _p(_pad(tb['sorted_pos'])), Q, Lt, int(enable), _p(cluster), _p(ncl))
    return st, cluster[:Lt], ncl[:Q]


def host_rows(c, tb, cluster, ncl, dedup=False):
    """-> (status, dict of ROW_KEYS + prob_base, N, M) of steps 4 and 5"""
    C, M0, Q = len(tb['pairs']), int(tb['pair_row_off'][-1]), c['Q']
    prob_base = np.concatenate([[0], np.cumsum(ncl)]).astype(np.int32)
    N = int(prob_base[-1])
    kp, pt, prob, first, slot, sel = (np.full(max(M0, 1), -1, np.int32) for _ in range(6))
    keep, poff, sizes = np.zeros(max(M0, 1), np.uint8), np.zeros(N + 1, np.int32), np.zeros(1, np.int32)
    st = host_lib().gf_covis_host_rows(_p(_pad(tb['pairs'])), _p(tb['pair_row_off']), C, M0, _p(_pad(c['ids'])), len(c['ids']), _p(c['kp_off']),
                                       c['n_images'], _p(_pad(c['pok'])), len(c['pok']), c['T'], _p(tb['list_off']), _p(_pad(cluster)),
                                       len(cluster), _p(prob_base), Q, N, int(dedup), _p(kp), _p(pt), _p(prob), _p(keep), _p(first), _p(slot),
                                       _p(sel), _p(poff), _p(sizes))
    M = int(sizes[0])
    return st, {'row_kp': kp[:M0], 'row_pt': pt[:M0], 'row_prob': prob[:M0], 'keep': keep[:M0], 'first_of': first[:M0], 'slot': slot[:M0],
                'sel': sel[:M], 'prob_off': poff, 'prob_base': prob_base, 'N': N, 'M': M}


SELECT_KEYS = ('winner', 'localized', 'R', 't', 'n_inliers', 'rounds', 'mask')


def host_select(prob_base, rs, row_prob, slot, min_inliers):
    """steps 8 and 9; rs: dict of numpy arrays valid, n_inliers, R, t, rounds, inliers"""
    Q, N, M, M0 = len(prob_base) - 1, len(rs['valid']), len(rs['inliers']), len(row_prob)
    win, loc, nin, rounds = (np.zeros(max(Q, 1), np.int32) for _ in range(4))
    R, t = np.zeros((max(Q, 1), 3, 3)), np.zeros((max(Q, 1), 3))
    is_win, mask = np.zeros(max(N, 1), np.uint8), np.zeros(max(M0, 1), np.uint8)
    a = {k: _pad(np.ascontiguousarray(rs[k])) for k in ('valid', 'n_inliers', 'R', 't', 'rounds', 'inliers')}
    host_lib().gf_covis_host_select(_p(np.ascontiguousarray(prob_base, np.int32)), Q, N, _p(a['valid']), _p(a['n_inliers']), _p(a['R']), _p(a['t']),
                                    _p(a['rounds']), _p(a['inliers']), M, _p(_pad(np.ascontiguousarray(row_prob, np.int32))),
                                    _p(_pad(np.ascontiguousarray(slot, np.int32))), M0, int(min_inliers), _p(win), _p(loc), _p(R), _p(t), _p(nin),
                                    _p(rounds), _p(is_win), _p(mask))
    return {'winner': win[:Q], 'localized': loc[:Q], 'R': R[:Q], 't': t[:Q], 'n_inliers': nin[:Q], 'rounds': rounds[:Q], 'mask': mask[:M0]}


# --------------------------------------------------------------------------------------------- two places that look alike
N_A, N_B = 6, 3                              # database cameras of place A and of place B
B_SHIFT = np.array([100.0, 0.0, 0.0])


def two_place_scene(seed=51, n_points=300, noise=0.5, share_a=0.7, share_b=0.5):
    """Place A: matcher_scene's cameras 0, 1, 3, 4, 6, 7 (database) and 2, 5 (queries) over n_points points.  Place B: N_B further database
    cameras looking at a rigid copy of A's points (rotated by 0.3 rad about y, moved by B_SHIFT): A and B share no point.  The first query
    has pairs with all nine database images; its matches into B are B's true projections of the copied structure, so B alone supports a
    consistent - and wrong - pose.  The second query has pairs with A's images only.  -> the dict of matcher_scene, with `place` per name."""
    rng = np.random.default_rng(seed)
    sc = TC.matcher_scene(seed, n_points, noise, share_a)
    K, R, t = TC.make_cameras(8, seed)
    c, s = np.cos(0.3), np.sin(0.3)
    G = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    XB = sc['X'] @ G.T + B_SHIFT                                         # the copy: X_B = G X + shift
    cams = [1, 4, 6][:N_B]
    RB = [R[i] @ G.T for i in cams]                                      # the same views of the copy: x_cam = R G^T (X_B - shift) + t
    tB = [t[i] - R[i] @ G.T @ B_SHIFT for i in cams]
    namesB = [f'/scene/db_b/{k}.png' for k in range(N_B)]
    uvB = np.array([[TC.project(K[i], RB[k], tB[k], x) + rng.normal(0, noise, 2) for x in XB] for k, i in enumerate(cams)]).astype(np.float32)
    pairs, results = list(sc['pairs']), list(sc['results'])
    add = [(namesB[a], namesB[b], uvB[a], uvB[b], share_a) for a in range(N_B) for b in range(a + 1, N_B)]
    q0 = sc['names'][TC.QUERIES[0]]
    add += [(q0, namesB[k], sc['uv'][TC.QUERIES[0]], uvB[k], share_b) for k in range(N_B)]
    for n0, n1, u0, u1, share in add:
        sel = np.sort(rng.choice(n_points, int(share * n_points), replace=False))
        m = np.concatenate([u0[sel], u1[sel]], 1)
        pairs.append((n0, n1)), results.append((m, m[:, :2].copy(), m[:, 2:].copy(), np.ones(len(sel), np.float32)))
    out = dict(sc, pairs=pairs, results=results, names=sc['names'] + namesB)
    out['intrinsics'] = dict(sc['intrinsics'], **{nm: K[i].reshape(3, 3).astype(np.float64) for nm, i in zip(namesB, cams)})
    out['db_poses'] = dict(sc['db_poses'], **{nm: (RB[k], tB[k]) for k, nm in enumerate(namesB)})
    out['place'] = {nm: ('B' if nm in namesB else 'A') for nm in out['names']}
    out['uv_b'], out['X_b'] = uvB, XB
    out['db_pair'] = np.array([a not in sc['queries'] and b not in sc['queries'] for a, b in pairs])
    return out


def database_only(cm, sc):
    """cm with the pairs between database images only, keypoints unchanged: what the database is triangulated from, as hloc reconstructs it
    before any query is matched.  (Through the first query's keypoints a track would otherwise join a point of A with its copy in B.)"""
    keep = np.flatnonzero(sc['db_pair'])
    return cm._replace(pair_images=cm.pair_images[keep], matches=[cm.matches[p] for p in keep])


def host_localize(cm, tt, names, intrinsics, cluster=True, dedup=False, thr=12.0, min_inliers=12, iters=512, refit=0):
    """matcher.localize_queries_sparse(covis_cluster=cluster, dedup=dedup) with the serial host builds in the place of the device: the
    bookkeeping of matcher._covis_tables, the host covisibility rule, the host absolute-pose RANSAC per problem (sample = the problem), the
    host selection.  -> dict(tables, rows, rs: per-problem arrays, sel: host_select's dict, n_clusters, cluster, p2d, p3d)"""
    import abspose_cases as AC
    from geoformer_amd import matcher
    tb = matcher._covis_tables(cm, tt, names)
    kp_off = np.concatenate([[0], np.cumsum([len(k) for k in cm.keypoints])]).astype(np.int32)
    c = {'n_images': len(cm.names), 'Q': len(names), 'T': len(tt.points), 'kp_off': kp_off, 'pok': np.concatenate(tt.point_of_keypoint).astype(np.int32),
         'obs_offsets': np.asarray(tt.obs_offsets, np.int32), 'obs_image': np.asarray(tt.obs_image, np.int32),
         'ids': np.concatenate([np.asarray(m, np.int32).reshape(-1, 2) for m in cm.matches])}
    st, cl, ncl = host_cluster(c, tb, enable=cluster)
    assert st == 0
    st, rows = host_rows(c, tb, cl, ncl, dedup=dedup)
    assert st == 0
    kps = np.concatenate([np.asarray(k, np.float32).reshape(-1, 2) for k in cm.keypoints])
    p2d, p3d = kps[rows['row_kp'][rows['sel']]], np.asarray(tt.points).astype(np.float32)[rows['row_pt'][rows['sel']]]
    N, M = rows['N'], rows['M']
    rs = {'valid': np.zeros(N, np.int32), 'n_inliers': np.zeros(N, np.int32), 'R': np.zeros((N, 3, 3)), 't': np.zeros((N, 3)),
          'rounds': np.zeros(N, np.int32), 'inliers': np.zeros(M, np.uint8)}
    query_of_prob = np.repeat(np.arange(len(names)), ncl)
    for k in range(N):
        a, b = rows['prob_off'][k], rows['prob_off'][k + 1]
        K9 = np.asarray(intrinsics[names[query_of_prob[k]]], np.float32).reshape(9)
        r = AC.host_ransac(p2d[a:b], p3d[a:b], thr=thr, iters=iters, sample=k, refit=refit, K9_=K9)
        rs['valid'][k], rs['n_inliers'][k], rs['R'][k], rs['t'][k], rs['rounds'][k] = r['valid'], r['n_inliers'], r['R'], r['t'], r['rounds']
        rs['inliers'][a:b] = r['inliers']
    sel = host_select(rows['prob_base'], rs, rows['row_prob'], rows['slot'], min_inliers)
    return {'tables': tb, 'rows': rows, 'rs': rs, 'sel': sel, 'n_clusters': ncl, 'cluster': cl, 'p2d': p2d, 'p3d': p3d,
            'query_of_prob': query_of_prob}
