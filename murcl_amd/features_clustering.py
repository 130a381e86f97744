"""Cluster every slide of a feature directory on the GPU k-means (``utils/clustering.py``: any feature width, up to 64 clusters):

    python -m murcl_amd.features_clustering --feat_dir DIR [--num_clusters 10] [--exist_ok] [--seeding {native,sklearn}] [--n_init N]

The command-line counterpart of the reference's wsi_processing/features_clustering.py: the same three flags, and for every
``DIR/<slide>.npz`` (array ``img_features`` [N,d]) the same two files, ``DIR/k-means-<K>/<slide>.npz`` (``features_cluster_indices``
[N,1]) and ``<slide>.json`` (K ascending patch-id lists, what ``WSIWithCluster`` reads as ``clusters_json_filepath``).  A slide whose
npz is already there is left alone unless ``--exist_ok`` is given; a slide with fewer patches than clusters is passed over.  Both
cases print the line the reference prints, so logs of the two tools can be compared.  There is no CPU path.

Two flags are this tool's own.  ``--seeding sklearn`` draws the k-means++ seeding from scikit-learn's random stream, so that the
files hold the partition the reference's ``KMeans(n_clusters, random_state=985)`` writes (``utils/clustering.py`` states when that
match is exact); ``--n_init`` sets the restarts (default: 3 with the native seeding, 1 with scikit-learn's, its ``n_init='auto'``;
a run of the reference made with scikit-learn before 1.4 had 10).  Without them the command writes what it always wrote.
"""
import argparse
import os

import numpy as np
import torch

from .utils import clustering as C


def build_parser(own_flags=False):
    """The reference's three flags; ``own_flags`` adds this tool's ``--seeding`` and ``--n_init`` (what ``main`` parses)."""
    p = argparse.ArgumentParser(prog="python -m murcl_amd.features_clustering", description=__doc__.split("\n\n")[0])
    p.add_argument("--feat_dir", type=str, default="", help="directory of per-slide feature files (<slide>.npz with an img_features array)")
    p.add_argument("--num_clusters", type=int, default=10, help="clusters per slide (1..64)")
    p.add_argument("--exist_ok", action="store_true", default=False, help="cluster again and overwrite slides that already have an output npz")
    if own_flags:
        p.add_argument("--seeding", type=str, default="native", choices=C.SEEDINGS,
                       help="k-means++ draws: torch's generator (native) or scikit-learn's random stream (sklearn: the reference's partition)")
        p.add_argument("--n_init", type=int, default=None, help="restarts (default: 3 with --seeding native, 1 with --seeding sklearn)")
    return p


def _slides(feat_dir):
    """(slide name, path) of the feature files directly under ``feat_dir``, by name."""
    return [(f[:-4], os.path.join(feat_dir, f)) for f in sorted(os.listdir(feat_dir))
            if f.endswith(".npz") and os.path.isfile(os.path.join(feat_dir, f))]


def run(args, device="cuda"):
    """Cluster the slides of ``args.feat_dir``. -> number of slides written."""
    if torch.device(device).type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"features_clustering on {device}: murcl_amd runs on MI355X only (no CPU path for its kernels)")
    K = args.num_clusters
    out_dir = os.path.join(args.feat_dir, f"k-means-{K}")
    os.makedirs(out_dir, exist_ok=True)
    slides = _slides(args.feat_dir)
    written = 0
    for pos, (slide, path) in enumerate(slides, 1):
        out_npz = os.path.join(out_dir, slide + ".npz")
        if os.path.exists(out_npz) and not args.exist_ok:
            print(f"{out_npz} is exists!")                                           # the reference's wording, kept for its logs
            continue
        with np.load(path) as archive:
            feats = np.asarray(archive["img_features"], dtype=np.float32)
        rows = feats.shape[0]
        if rows < K:
            print(f"{slide}'s number of features < number of clusters, can't clustering.")    # likewise
            continue
        labels = C.clustering(feats, K, filepath=out_npz, device=device, seeding=getattr(args, "seeding", "native"),
                              n_init=getattr(args, "n_init", None))
        C.save_to_json(labels, K, filepath=os.path.join(out_dir, slide + ".json"))
        written += 1
        print(f"[{pos}/{len(slides)}] {slide}: {rows} patches x {feats.shape[1]} -> {K} clusters", flush=True)
    return written


def main(argv=None):
    return run(build_parser(own_flags=True).parse_args(argv))


if __name__ == "__main__":
    main()
