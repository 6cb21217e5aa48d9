from .engine import (  # noqa: F401
    ESConfig,
    ESEngine,
    eval_matrix_reference,
    init_theta,
    make_env_params,
)
from .cartpole import CartPoleESEngine  # noqa: F401
from .ga import GAConfig, GAEngine  # noqa: F401
from .lmmaes import LMMAESConfig, LMMAESEngine  # noqa: F401
from .lstm import LSTMESEngine, init_theta_lstm  # noqa: F401
from .lstm_cartpole import LSTMCartPoleESEngine  # noqa: F401
from .map_elites import MapElitesConfig, MapElitesEngine  # noqa: F401
from .novelty import NoveltyConfig, NoveltyESEngine  # noqa: F401
from .population import ESPopulation  # noqa: F401
from .recurrent import RecurrentESEngine, init_theta_gru  # noqa: F401
from .safe_ga import SafeGAConfig, SafeGAEngine  # noqa: F401
from .snes import SNESConfig, SNESEngine  # noqa: F401
from .wide import WideESEngine, init_theta_wide  # noqa: F401
from .poet import (  # noqa: F401
    apply_transfers,
    minimal_criterion,
    propose_children,
    reproduce,
    select_children,
    select_transfers,
    transfer_matrix,
)
