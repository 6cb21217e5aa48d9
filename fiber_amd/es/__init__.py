from .engine import (  # noqa: F401
    ESConfig,
    ESEngine,
    eval_matrix_reference,
    init_theta,
    make_env_params,
)
from .ga import GAConfig, GAEngine  # noqa: F401
from .map_elites import MapElitesConfig, MapElitesEngine  # noqa: F401
from .novelty import NoveltyConfig, NoveltyESEngine  # noqa: F401
from .population import ESPopulation  # noqa: F401
from .safe_ga import SafeGAConfig, SafeGAEngine  # noqa: F401
from .snes import SNESConfig, SNESEngine  # noqa: F401
from .poet import (  # noqa: F401
    apply_transfers,
    minimal_criterion,
    propose_children,
    reproduce,
    select_children,
    select_transfers,
    transfer_matrix,
)
