"""Command-line surface of the reference trainer (MF/parse.py:3-117), kept flag-for-flag so that the commands
in the reference README (README.md:41,69,93) run unchanged against `python -m pda_amd.train_new_api`.

Flags the reference marks "not used" are accepted and ignored (they still have to parse).  A few flags are
additions of this implementation and default to the reference's behaviour; they are listed last.
"""
from __future__ import annotations

import argparse

# (name, type, default, help)   -- type None means "nargs='?' string" exactly like the reference
_REFERENCE_FLAGS = [
    ("data_path", None, "./data/", "root directory that holds <dataset>/"),
    ("dataset", None, "kwai", "dataset directory name"),
    ("source", None, "normal", "(unused)"),
    ("train", None, "normal", "normal (BPRMF) | s_condition (PD/PDA) | temp_pop | dice | ips | macr | ssm (the sampled-softmax loss, --ssm_negs / --ssm_tau / --ssm_norm) | ials (implicit ALS, --ials_alpha0 / --ials_nu; no sampler, no optimiser) | pcc (BPR plus the popularity-correlation regulariser, --pcc_gamma / --pcc_on / --pcc_pop) | dau (the DirectAU alignment + uniformity loss, --dau_gamma / --dau_t / --dau_same / --dau_rank; no negatives) | warp (the WARP loss: the rank-weighted hinge on the first of --warp_max_trials uniform candidates that violates --warp_margin, --warp_weight; fp32 tables, the device sampler, one GPU)"),
    ("test", None, "normal", "normal (BPRMF/BPRMF-A) | s_condition (PD/PDA) | temp_pop | dice | ips | macr | ssm (the raw head of an SSM model alone) | ials (the raw head of an iALS model alone) | pcc (the raw head of a PCC model alone) | dau (the main head of a DirectAU model alone)"),
    ("valid_set", None, "test", "test | valid"),
    ("save_dir", None, "/data/zyang/save_model/", "checkpoint root"),
    ("alpha", float, 1e-3, "MACR (--train macr): weight of the item-branch loss L_I; otherwise unused (appears in the checkpoint directory name)"),
    ("beta", float, 1e-3, "MACR: weight of the user-branch loss L_U; otherwise unused"),
    ("pc_alpha", float, 0.1, "BPR-PC (python -m pda_amd.bpr_pc): weight alpha of the popularity compensation"),
    ("pc_beta", float, 0.1, "BPR-PC: beta of the compensation C = (beta s + 1 - beta) / pop"),
    ("exp_init_values", float, 0.1, "(unused)"),
    ("pop_exp", float, 0.1, "popularity exponent gamma"),
    ("early_stop", int, 1, "1: stop when recall@Ks[0] stalls"),
    ("need_save", int, 1, "(unused)"),
    ("cores", int, 1, "(unused)"),
    ("verbose", int, 1, "print every `verbose` epochs between evaluations"),
    ("epoch", int, 400, "number of epochs"),
    ("load_epoch", int, 400, "(unused)"),
    ("embed_size", int, 64, "embedding width d"),
    ("batch_size", int, 1024, "triplets per step"),
    ("Ks", None, "[20]", "python list literal of cut-offs, max 50"),
    ("epochs", None, "[]", "(unused)"),
    ("regs", float, 1e-5, "L2 coefficient"),
    ("fregs", float, 1e-5, "(unused)"),
    ("c", float, 10.0, "MACR: the counterfactual constant c of (y - c) s_i s_u when --check_c 0; otherwise unused"),
    ("train_c", str, "val", "(unused)"),
    ("lr", float, 1e-3, "learning rate"),
    ("wd", float, 1e-5, "(overwritten by --regs, MF/train_new_api.py:1020)"),
    ("model", None, "mf", "mf (matrix factorisation) | lightgcn (the LightGCN backbone, --gcn_layers; --train normal | s_condition)"),
    ("skew", int, 0, "(unused)"),
    ("model_type", None, "o", "(unused)"),
    ("devide_ratio", float, 0.8, "(unused)"),
    ("save_flag", int, 1, "1: also checkpoint every 50 epochs"),
    ("pop_used", int, -2, "(unused)"),
    ("cuda", str, "1", "visible GPU id (HIP_VISIBLE_DEVICES)"),
    ("pretrain", int, 0, "only 0 is implemented"),
    ("check_c", int, 1, "MACR: 1 searches c over linspace(--start, --end, --step) at every evaluation, 0 uses --c; otherwise unused"),
    ("log_interval", int, 10, "evaluate every this many epochs"),
    ("pop_wd", float, 0.0, "(unused)"),
    ("base", float, -1.0, "(unused)"),
    ("cf_pen", float, 1.0, "(unused)"),
    ("saveID", None, "", "suffix of the checkpoint directory"),
    ("user_min", int, 1, "(unused)"),
    ("user_max", int, 1000, "(unused)"),
    ("data_type", None, "ori", "only 'ori' is implemented"),
    ("imb_type", None, "exp", "(unused)"),
    ("top_ratio", float, 0.1, "(unused)"),
    ("lam", float, 1.0, "(unused)"),
    ("check_epoch", None, "all", "(unused)"),
    ("start", float, -1.0, "MACR: first value of the search over c; otherwise unused"),
    ("end", float, 1.0, "MACR: last value of the search over c; otherwise unused"),
    ("step", int, 20, "MACR: number of values of the search over c; otherwise unused"),
    ("out", int, 0, "(unused)"),
]

_EXTENSION_FLAGS = [
    ("optimizer", str, "adam", "adam = TF-1.14 dense-decay Adam (reference, MF/model_api.py:83) | lazy_adam | sgd (exact mini-batch step) | sgd_fused (one launch, asynchronous in-kernel update)"),
    ("adam_sweep", str, "auto", "how --optimizer adam applies the reference's dense decay: sweep = one pass over both tables per step | replay = the same arithmetic without the sweep (idle rows replay their decay when next needed; bit-identical after the sync) | replay_fast = that catch-up to 1e-6 instead of bit for bit (~4x less arithmetic; explicit opt-in) | auto = sweep up to 64 MB of tables, the bit-identical replay above"),
    ("sampler", str, "device", "device = HIP counter-based sampler | host = the reference's Python generators"),
    ("table_dtype", str, "f32", "f32 | bf16 (BASELINE config 5): bf16 embedding tables for the forward pass and the evaluation, fp32 masters take the updates"),
    ("deterministic", int, 0, "1: the run is a function of its flags and data alone, bit for bit -- gradients summed in the order of the batch's plan and metrics in wave order instead of with float atomics (adam, lazy_adam, sgd on one GPU, fp32 tables under Adam; not temp_pop)"),
    ("eval_block", int, 262144, "users per score+top-K launch (the reference always uses 2048, MF/train_new_api.py:703); large blocks balance the early-terminating sweep: 92 M users/s at 65536, 109 M at 262144 (C3)"),
    ("topk_max", int, 50, "columns of every ranking (the reference's graph constant, MF/train_new_api.py:594: 50); 1 .. 1024.  Above 54 the lists come from the deep path (include/pda_hip_deep.h): --train normal | s_condition on one GPU"),
    ("export_out", str, "", "python -m pda_amd.export_topk: the .npz file that receives users, idx and val"),
    ("xq_lambda", float, 0.5, "xQuAD (python -m pda_amd.xquad): weight lambda of the diversification term, 0 .. 1 (0 leaves the BPRMF ranking)"),
    ("xq_candidates", int, 1000, "xQuAD: candidates per user the re-ranking selects from, max(Ks) .. 1024 (above 54 they come from the deep path)"),
    ("xq_head_share", float, 0.8, "xQuAD: the short head is the most popular items that hold this share of the train interactions, strictly inside 0 .. 1"),
    ("xq_variant", str, "smooth", "xQuAD: smooth | binary"),
    ("cp_lambda", float, 0.5, "calibrated popularity (python -m pda_amd.calib): weight lambda of the divergence between the list's and the user's popularity mix, 0 .. 1 (0 leaves the ranking it re-ranks)"),
    ("cp_candidates", int, 1000, "calibrated popularity: candidates per user the re-ranking selects from, max(Ks) .. 1024, cut to the catalogue's size (above 54 they come from the deep path)"),
    ("cp_cuts", str, "[0.2,0.8]", "calibrated popularity: the popularity groups, a list literal of up to 7 strictly increasing cuts inside 0 .. 1 -- shares of the train interactions, the items taken from the most popular down (the default: head, mid and tail)"),
    ("cp_div", str, "js", "calibrated popularity: js = Jensen-Shannon divergence, log2 (Abdollahpouri et al., UMAP 2021) | kl = KL divergence from the list smoothed by --cp_alpha (Steck, RecSys 2018)"),
    ("cp_alpha", float, 0.01, "calibrated popularity (--cp_div kl): the share alpha of the profile mixed into the list's distribution, strictly inside 0 .. 1"),
    ("bias_report", int, 0, "1: after every metrics line, `||--- bias@K` lines on what the lists do to popularity bias -- recommendation rate, hit share and recall per popularity group, ARP, coverage, Gini, APLT (pda_amd/exposure.py; the head of APLT is --xq_head_share); one GPU; 0 | 1"),
    ("bias_groups", int, 10, "--bias_report: popularity groups of the items, 1 .. 64 (group 0 = the most popular)"),
    ("bias_group_by", str, "interactions", "--bias_report: interactions = groups of equal train interactions | items = groups of equal item counts"),
    ("rank_report", int, 0, "1: after every metrics line (and the bias lines), `||--- rank` lines from the exact position of every held-out item in its user's masked full-catalogue ranking -- AUC, MRR, mean percentile rank, mean and median rank, recall@K and hit@K at --rank_ks, and MPR, median rank and recall@K per popularity group of the held-out item (--bias_groups, --bias_group_by); include/pda_hip_rank.h, pda_amd/rank_report.py; the raw and the popularity head on one GPU (not --train temp_pop | macr); accepted with --deterministic 1 (integer counts); 0 | 1"),
    ("rank_ks", str, "[50, 1000]", "--rank_report: the cut-offs of its recall@K and hit@K, a list literal like --Ks; any positive K (positions are exact at every depth, beyond --topk_max and 1024 too)"),
    ("gcn_layers", int, 3, "LightGCN (--model lightgcn): propagation layers L, 0 .. 4; the final tables are the mean of the L + 1 layers (0: the ego tables alone, matrix factorisation through this path)"),
    ("ials_alpha0", float, 0.1, "iALS (--train ials, include/pda_hip_ials.h): weight alpha0 of the unobserved pairs, >= 0.  --regs is lambda (> 0); --lr, --optimizer, --adam_sweep, --sampler and --batch_size (for training) are unused by iALS"),
    ("ials_nu", float, 1.0, "iALS: frequency scaling of the regulariser, lambda (n + alpha0 n_other)^nu per row, 0 .. 1 (0: plain L2)"),
    ("ials_solver", str, "exact", "iALS: exact = every row solved exactly, a d x d system per row (--embed_size 32 | 64 | 128) | block = iALS++ (include/pda_hip_ialspp.h): per epoch one exact step on each block of --ials_block coordinates, users then items, --embed_size 32 | 64 | 128 | 256.  A block step starts from the tables as they stand, so their initialisation matters (the exact solver forgets it after one half-sweep) and an epoch converges more slowly than an exact one"),
    ("ials_item_power", float, 0.0, "iALS (either solver; include/pda_hip_ials_itemw.h): item-weighted unobserved pairs (the eALS weighting).  The unobserved pairs of item i weigh alpha0 w_i with w_i ~ (c_i + 1)^power of the item's distinct train pairs c_i, normalised to mean 1, 0 .. 4; 0 (default): every w_i is 1, the unweighted model, bit for bit"),
    ("ials_block", int, 32, "iALS (--ials_solver block): the block size k, 32 | 64 | 128; it has to divide --embed_size (k = --embed_size is the exact solve started from the current tables)"),
    ("pcc_gamma", float, 1.0, "PCC (--train pcc, include/pda_hip_pcc.h): weight gamma of the penalty gamma r^2, r the Pearson correlation over the batch between a score and the popularity of the positive, >= 0 (0: the BPR loss, r is still reported).  The default is UNTUNED: nothing here has the data sets"),
    ("pcc_on", str, "pos", "PCC: the score that is correlated with the positive's popularity.  pos = the score of the observed pair (Zhu et al., WSDM'21) | margin = the pairwise margin, positive score minus negative score"),
    ("pcc_pop", str, "count", "PCC: the popularity of an item.  count = its train interactions n_i | log = log1p(n_i)"),
    ("dau_gamma", float, 1.0, "DirectAU (--train dau, include/pda_hip_dau.h): weight gamma of the uniformity term gamma (uni_U + uni_I) / 2 beside the alignment term, >= 0 (0: alignment alone).  The default is UNTUNED: nothing here has the data sets"),
    ("dau_t", float, 2.0, "DirectAU: temperature t of the uniformity kernel exp(-t |x - y|^2) on the unit sphere, 0 < t <= 20"),
    ("dau_same", str, "keep", "DirectAU: pairs of batch rows that carry the same user (or the same item).  keep = they count, at distance 0 (a pairwise distance over the batch as it stands) | drop = they are left out of the uniformity mean"),
    ("dau_rank", str, "raw", "DirectAU: what the lists rank by.  raw = the dot product of the raw tables | cosine = of the row-normalised tables (the quantity the loss trained; the path --ssm_norm 1 takes)"),
    ("neg_sampler", str, "uniform", "where a triplet's negative comes from: uniform = one uniform draw outside the user's train items (the reference) | dns = dynamic hard-negative sampling, DNS(M, N): one of the --dns_topn best-scoring of --dns_candidates uniform draws under the current tables (include/pda_hip_dns.h; --train normal | s_condition, fp32 tables, the device sampler, one GPU) | pop = popularity-weighted negatives, q_i ~ (c_i + 1)^--neg_pop_power with c_i the item's train pairs, drawn through an alias table and rejected against the user's train items like the uniform draw (include/pda_hip_negpop.h; --train normal | s_condition | ssm with --ssm_source sampled, the device sampler, one GPU)"),
    ("neg_pop_power", float, 0.75, "--neg_sampler pop: the power beta of q_i ~ (c_i + 1)^beta, 0 .. 4 (0: the uniform sampler's batches, bit for bit; 0.75: the unigram^0.75 of word2vec; 1: in proportion to popularity)"),
    ("dns_candidates", int, 16, "DNS (--neg_sampler dns): candidates M drawn and scored per triplet, 1 .. 256 (1: the uniform sampler's batches, bit for bit)"),
    ("dns_topn", int, 1, "DNS: the negative is drawn uniformly from the N best of the M candidates, 1 .. --dns_candidates (1: the best one, the classic DNS)"),
    ("warp_max_trials", int, 64, "WARP (--train warp, include/pda_hip_warp.h): the uniform candidates T a triplet may try, 1 .. 256; its negative is the first one that violates the margin, the number of tries N estimates the positive's rank, floor((n_items - 1) / N)"),
    ("warp_margin", float, 1.0, "WARP: the margin of the hinge, margin - (u.pos - u.neg); a candidate violates when that is > 0.  A finite number.  The default is UNTUNED: nothing here has the data sets"),
    ("warp_weight", str, "harmonic", "WARP: the weight of a triplet as a function of the estimated rank.  harmonic = 1 + 1/2 + .. + 1/rank (WSABIE) | log = log(max(1, rank)) (LightFM's form; 0 at rank 1) | none = 1 (the plain hinge on the first violator)"),
    ("ssm_source", str, "sampled", "SSM (--train ssm): where a row's negatives come from.  sampled = --ssm_negs uniform draws per row | batch = the other rows' positives (in-batch softmax, include/pda_hip_inbatch.h: --batch_size - 1 shared negatives per row, --batch_size in 2 .. 16384) | all = every item of the catalogue, no sampling (the exact softmax both estimate, include/pda_hip_fullsm.h: --batch_size in 1 .. 16384)"),
    ("ssm_logq", int, 1, "SSM with --ssm_source batch: 1 subtracts log q_i, the log-probability that item i sits in a column of the batch, from every logit of column item i, the positive's own included (logQ correction of the popularity-skewed in-batch negatives); 0 | 1; with --ssm_source sampled it acts under --neg_sampler pop (log q_i of the popularity proposal, the same convention) and is unused under --neg_sampler uniform, where the correction is a constant that cancels in the softmax; unused with --ssm_source all (nothing is sampled, so there is nothing to correct)"),
    ("ssm_mask_train", int, 1, "SSM with --ssm_source batch: 1 leaves a column out of a row's softmax when its item is a train item of the row's user (the sampled path rejects the same items when it draws); with --ssm_source all: 1 leaves the user's other train items out of the row's softmax over the catalogue, 0 keeps every item; 0 | 1"),
    ("ssm_negs", int, 64, "SSM (--train ssm): sampled negatives per row of the softmax, 1 .. 256; unused with --ssm_source batch and with --ssm_source all"),
    ("ssm_tau", float, 0.1, "SSM: the temperature tau of the logits, > 0"),
    ("ssm_norm", int, 1, "SSM: 1 takes the logits on cosine similarity (rows normalised to length 1, in training and in the lists), 0 on the raw dot product; 0 | 1"),
    ("ips_clip", float, 0.0, "IPS (--train ips): clip the inverse propensity weights at this value (IPS-C); 0: no clip"),
    ("ips_norm", int, 0, "IPS: 1 divides a batch's weighted loss by the sum of its weights instead of the batch size (IPS-CN, with --ips_clip); 0 | 1"),
    ("dice_int_weight", float, 0.1, "DICE (--train dice): weight of the interest loss L_int"),
    ("dice_con_weight", float, 0.1, "DICE: weight of the conformity loss L_con"),
    ("dice_dis_pen", float, 0.01, "DICE: weight of the discrepancy term (the loss takes -dice_dis_pen * L_dis)"),
    ("dice_dis_loss", str, "l1", "DICE: the discrepancy between the interest and the conformity embeddings, l1 | l2"),
    ("dice_margin", float, 40.0, "DICE: the popularity margin M of the negative sampler (PNSM), in train interactions"),
    ("dice_margin_decay", float, 0.9, "DICE: M is multiplied by this at the start of every epoch after the first"),
    ("dice_loss_decay", float, 0.9, "DICE: dice_int_weight and dice_con_weight are multiplied by this at the start of every epoch after the first"),
]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Run pop_bias (PDA BPR-MF) on MI355X.")
    for name, typ, default, hlp in _REFERENCE_FLAGS + _EXTENSION_FLAGS:
        if typ is None:
            p.add_argument("--" + name, nargs="?", default=default, help=hlp)
        else:
            p.add_argument("--" + name, type=typ, default=default, help=hlp)
    return p


def parse_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def reference_flag_names():
    return [f[0] for f in _REFERENCE_FLAGS]
