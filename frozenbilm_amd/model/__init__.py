"""Model factory with the reference's signatures (model/__init__.py:14-112)."""
from .adapter import Adapter
from .bert import BertConfig, BertForMaskedLM
from .config import DebertaV2Config
from .deberta import LORA_DEFAULT_TARGETS, DebertaV2ForMaskedLM, MaskedLMOutput


def build_model(args, config=None):
    """``build_model(args)`` of the reference for the DeBERTa and BERT branches (model/__init__.py:15-62).

    No hub / checkpoint access exists on the MI355X box, so the configuration is the literal DeBERTa-v2-XLarge one
    (BERT-Base / BERT-Large for names with "bert" but not "deberta") unless ``config`` (ours, a transformers config, or a
    dict) is given; weights come from ``load_state_dict`` (reference key names) or stay at their seeded initialisation
    (``--scratch`` behaviour).
    """
    name = getattr(args, "model_name", "deberta-v2-xlarge")
    if "deberta" not in name and "bert" in name:
        # model/__init__.py:48-62: the reference's BERT has no adapters and is always loaded pretrained
        assert (not args.ds_factor_ff) and (not args.ds_factor_attn) and (not getattr(args, "scratch", False))
        if config is not None:
            cfg = BertConfig.from_any(config)
        else:
            cfg = BertConfig.large() if "large" in name else BertConfig.base()
        return BertForMaskedLM(
            cfg,
            features_dim=args.features_dim if getattr(args, "use_video", True) else 0,
            max_feats=args.max_feats,
            freeze_lm=getattr(args, "freeze_lm", True),
            freeze_mlm=getattr(args, "freeze_mlm", True),
            ft_ln=getattr(args, "ft_ln", True),
            n_ans=getattr(args, "n_ans", 0),
            freeze_last=getattr(args, "freeze_last", True),
            lora_rank=getattr(args, "lora_rank", 0),
            lora_alpha=getattr(args, "lora_alpha", None),
            lora_targets=getattr(args, "lora_targets", LORA_DEFAULT_TARGETS),
            n_prompt=getattr(args, "n_prompt", 0),
            prompt_depth=getattr(args, "prompt_depth", 1),
        )
    if "deberta" not in name:
        raise NotImplementedError(f"only the DeBERTa-v2 and BERT paths are implemented (model_name={name!r})")
    cfg = DebertaV2Config.from_any(config) if config is not None else DebertaV2Config()
    return DebertaV2ForMaskedLM(
        cfg,
        features_dim=args.features_dim if getattr(args, "use_video", True) else 0,
        max_feats=args.max_feats,
        freeze_lm=getattr(args, "freeze_lm", True),
        freeze_mlm=getattr(args, "freeze_mlm", True),
        ft_ln=getattr(args, "ft_ln", True),
        ds_factor_attn=args.ds_factor_attn,
        ds_factor_ff=args.ds_factor_ff,
        dropout=args.dropout,
        n_ans=getattr(args, "n_ans", 0),
        freeze_last=getattr(args, "freeze_last", True),
        lora_rank=getattr(args, "lora_rank", 0),
        lora_alpha=getattr(args, "lora_alpha", None),
        lora_targets=getattr(args, "lora_targets", LORA_DEFAULT_TARGETS),
        n_prompt=getattr(args, "n_prompt", 0),
        prompt_depth=getattr(args, "prompt_depth", 1),
    )


def get_tokenizer(args):
    """Pass-through to transformers' DebertaV2Tokenizer / BertTokenizer (model/__init__.py:94-112); needs local files."""
    if "deberta" not in args.model_name and "bert" in args.model_name:
        from transformers import BertTokenizer

        return BertTokenizer.from_pretrained(args.model_name, local_files_only=True)
    from transformers import DebertaV2Tokenizer

    return DebertaV2Tokenizer.from_pretrained(args.model_name, local_files_only=True)
