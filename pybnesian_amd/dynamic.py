"""Dynamic Bayesian networks on top of the same kernels: DynamicDataFrame (dataset/dynamic_dataset.{hpp,
cpp}), the Dynamic* adaptators of scores and independence tests (learning/scores/scores.hpp:74-101,
learning/independences/independence.hpp:42-77), DynamicBayesianNetwork (models/DynamicBayesianNetwork.{hpp,cpp}) and DMMHC
(learning/algorithms/dmmhc.cpp).  Everything here is index bookkeeping: the static network is learned on the lagged
"static" table, the transition network - a conditional network whose interface nodes are the lagged variables - on the
"transition" table, with the scores, tests, MMPC and hill-climb of this package."""
import numpy as np

from .network_pass import CLG, GAUSSIAN, one_pass
from .dataset import as_record_batch
from .models import BayesianNetwork, GaussianNetworkType


def temporal_name(name, slice_index):   # util/temporal.cpp:5-7
    return f"{name}_t_{slice_index}"


def temporal_names(variables, offset_slice, markovian_order):   # util/temporal.cpp:9-23
    return [temporal_name(v, i) for v in variables for i in range(offset_slice, markovian_order + 1)]


def _temporal_slice(rb, slice_index, slice_offset, markovian_order):   # dynamic_dataset.cpp:16-33
    import pyarrow as pa

    new_length = rb.num_rows - markovian_order
    offset = markovian_order - slice_index
    sl = rb.slice(offset, new_length)
    return pa.RecordBatch.from_arrays(sl.columns, names=[temporal_name(n, slice_index + slice_offset) for n in rb.schema.names])


def _concat_columns(batches):
    import pyarrow as pa

    cols, names = [], []
    for b in batches:
        cols += b.columns
        names += b.schema.names
    return pa.RecordBatch.from_arrays(cols, names=names)


def static_table(df, markovian_order):   # create_static_df, dynamic_dataset.cpp:45-71
    import pyarrow as pa

    rb = as_record_batch(df)
    if markovian_order == 1:
        return pa.RecordBatch.from_arrays(rb.columns, names=[temporal_name(n, 1) for n in rb.schema.names])
    return _concat_columns([_temporal_slice(rb, i, 1, markovian_order - 1) for i in range(markovian_order)])


def transition_table(df, markovian_order):   # create_temporal_slices + create_transition_df, :35-43, :73-85
    rb = as_record_batch(df)
    return _concat_columns([_temporal_slice(rb, i, 0, markovian_order) for i in range(markovian_order + 1)])


class DynamicDataFrame:
    def __init__(self, df, markovian_order):
        if markovian_order < 1:
            raise ValueError("Markovian order must be at least 1.")
        self._origin = as_record_batch(df)
        if self._origin.num_rows <= markovian_order:
            raise ValueError("Not enough rows for this markovian order.")
        self._order = int(markovian_order)
        self._static = static_table(self._origin, self._order)
        self._transition = transition_table(self._origin, self._order)

    def markovian_order(self):
        return self._order

    def num_variables(self):
        return self._origin.num_columns

    def num_rows(self):
        return self._transition.num_rows

    def num_columns(self):
        return self._transition.num_columns

    def origin_df(self):
        return self._origin

    def static_df(self):
        return self._static

    def transition_df(self):
        return self._transition

    def temporal_slice(self, index):
        if not 0 <= index <= self._order:
            raise ValueError(f"slice_index must be an index between 0 and {self._order}")
        return _temporal_slice(self._origin, index, 0, self._order)

    def variable_names(self):
        return list(self._origin.schema.names)


class _DynamicAdaptator:
    """DynamicAdaptator<Base> (dataset/dynamic_dataset.hpp): one Base on the static table, one on the transition table."""

    def __init__(self, base, ddf, *args, **kwargs):
        if not isinstance(ddf, DynamicDataFrame):
            raise ValueError("A DynamicDataFrame is needed.")
        self._ddf = ddf
        self._static = base(ddf.static_df(), *args, **kwargs)
        self._transition = base(ddf.transition_df(), *args, **kwargs)

    def variable_names(self):
        return self._ddf.variable_names()

    def has_variables(self, variables):
        names = set(self._ddf.variable_names())
        variables = [variables] if isinstance(variables, str) else variables
        return all(v in names for v in variables)

    def markovian_order(self):
        return self._ddf.markovian_order()


def _pure(cls, name):
    def fn(self, *args, **kwargs):
        raise NotImplementedError(f'Tried to call pure virtual function "{cls}::{name}"')
    return fn


class DynamicScore:
    """learning/scores/scores.hpp:74-101: subclass and implement has_variables, static_score, transition_score."""

    has_variables = _pure("DynamicScore", "has_variables")
    static_score = _pure("DynamicScore", "static_score")
    transition_score = _pure("DynamicScore", "transition_score")


class DynamicIndependenceTest:
    """learning/independences/independence.hpp: subclass and implement num_variables, variable_names, name,
    has_variables, markovian_order, static_tests, transition_tests."""

    num_variables = _pure("DynamicIndependenceTest", "num_variables")
    variable_names = _pure("DynamicIndependenceTest", "variable_names")
    name = _pure("DynamicIndependenceTest", "name")
    has_variables = _pure("DynamicIndependenceTest", "has_variables")
    markovian_order = _pure("DynamicIndependenceTest", "markovian_order")
    static_tests = _pure("DynamicIndependenceTest", "static_tests")
    transition_tests = _pure("DynamicIndependenceTest", "transition_tests")


class DynamicScoreAdaptator(_DynamicAdaptator, DynamicScore):
    def static_score(self):
        return self._static

    def transition_score(self):
        return self._transition


class DynamicIndependenceTestAdaptator(_DynamicAdaptator, DynamicIndependenceTest):
    def num_variables(self):
        return len(self._ddf.variable_names())

    def name(self, index):
        return self._ddf.variable_names()[index]

    def static_tests(self):
        return self._static

    def transition_tests(self):
        return self._transition


def _adaptator(kind, base_name):
    def make(ddf, *args, **kwargs):
        import pybnesian_amd as pbn

        return kind(getattr(pbn, base_name), ddf, *args, **kwargs)

    make.__name__ = "Dynamic" + base_name
    make.__doc__ = f"Dynamic{base_name}(ddf, ...): {base_name} on the static and on the transition table of a DynamicDataFrame."
    return make


DynamicBIC = _adaptator(DynamicScoreAdaptator, "BIC")
DynamicBGe = _adaptator(DynamicScoreAdaptator, "BGe")
DynamicBDe = _adaptator(DynamicScoreAdaptator, "BDe")
DynamicCVLikelihood = _adaptator(DynamicScoreAdaptator, "CVLikelihood")
DynamicHoldoutLikelihood = _adaptator(DynamicScoreAdaptator, "HoldoutLikelihood")
DynamicValidatedLikelihood = _adaptator(DynamicScoreAdaptator, "ValidatedLikelihood")
DynamicLinearCorrelation = _adaptator(DynamicIndependenceTestAdaptator, "LinearCorrelation")
DynamicMutualInformation = _adaptator(DynamicIndependenceTestAdaptator, "MutualInformation")
DynamicChiSquare = _adaptator(DynamicIndependenceTestAdaptator, "ChiSquare")
DynamicKMutualInformation = _adaptator(DynamicIndependenceTestAdaptator, "KMutualInformation")
DynamicRCoT = _adaptator(DynamicIndependenceTestAdaptator, "RCoT")


class DynamicBayesianNetworkBase:
    """models/DynamicBayesianNetwork.hpp:20-60: the abstract interface DynamicBayesianNetwork implements."""


class DynamicBayesianNetwork(DynamicBayesianNetworkBase):
    """models/DynamicBayesianNetwork.hpp: a static network over the lagged variables v_t_1 .. v_t_order and a conditional
    transition network over v_t_0 with the lagged variables as interface nodes."""

    def __init__(self, *args, **kwargs):
        """The reference's overloads (pybindings_models.cpp:2590-2665): (type, variables, markovian_order) and
        (variables, markovian_order, static_bn, transition_bn); `bn_type=` as keyword also accepted."""
        from .models import BayesianNetworkType

        args = list(args)
        bn_type = kwargs.pop("bn_type", None)
        if args and isinstance(args[0], BayesianNetworkType):
            bn_type = args.pop(0)
        names = ["variables", "markovian_order", "static_bn", "transition_bn", "bn_type"]
        for k, v in zip(names, args):
            kwargs[k] = v
        variables, markovian_order = kwargs["variables"], kwargs["markovian_order"]
        static_bn, transition_bn = kwargs.get("static_bn"), kwargs.get("transition_bn")
        bn_type = kwargs.get("bn_type", bn_type)
        self._variables = list(variables)
        self._order = int(markovian_order)
        if self._order < 1:
            raise ValueError("Markovian order must be at least 1.")
        if (static_bn is None) != (transition_bn is None):
            raise ValueError("Static and transition Bayesian networks must be given together.")
        bn_type = bn_type if bn_type is not None else (static_bn.type() if static_bn is not None else GaussianNetworkType())
        static_nodes = temporal_names(self._variables, 1, self._order)
        transition_nodes = temporal_names(self._variables, 0, 0)
        if static_bn is None:
            static_bn = bn_type.new_bn(static_nodes)
            transition_bn = bn_type.new_cbn(transition_nodes, static_nodes)
        if static_bn.type() != transition_bn.type():
            raise ValueError("Static and transition Bayesian networks do not have the same type.")
        if set(static_bn.nodes()) != set(static_nodes):
            raise ValueError("Static Bayesian network must contain the nodes: " + ", ".join(static_nodes))
        if set(transition_bn.nodes()) != set(transition_nodes) or set(transition_bn.interface_nodes()) != set(static_nodes):
            raise ValueError("Transition Bayesian network has the wrong nodes / interface nodes.")
        self._static, self._transition = static_bn, transition_bn

    def variables(self):
        return list(self._variables)

    def num_variables(self):
        return len(self._variables)

    def contains_variable(self, name):
        return name in self._variables

    def add_variable(self, name):
        """DynamicBayesianNetwork::add_variable (DynamicBayesianNetwork.hpp:100-120): its lagged copies join the static
        network and the transition network's interface, name_t_0 the transition network's nodes."""
        if name in self._variables:
            raise ValueError(f"Cannot add variable {name} because a variable with the same name already exists.")
        self._variables.append(name)
        for i in range(1, self._order + 1):
            self._static.add_node(temporal_name(name, i))
            self._transition.add_interface_node(temporal_name(name, i))
        self._transition.add_node(temporal_name(name, 0))

    def remove_variable(self, name):
        if name not in self._variables:
            raise ValueError(f"Variable {name} not present in the dynamic Bayesian network.")
        self._variables.remove(name)
        for i in range(1, self._order + 1):
            self._static.remove_node(temporal_name(name, i))
            self._transition.remove_interface_node(temporal_name(name, i))
        self._transition.remove_node(temporal_name(name, 0))

    def markovian_order(self):
        return self._order

    def static_bn(self):
        return self._static

    def transition_bn(self):
        return self._transition

    def type(self):
        return self._transition.type()

    def fit(self, df):
        ddf = df if isinstance(df, DynamicDataFrame) else DynamicDataFrame(df, self._order)
        self._static.fit(ddf.static_df())
        self._transition.fit(ddf.transition_df())

    def fitted(self):
        return self._static.fitted() and self._transition.fitted()

    def _check(self, rb):
        if not self.fitted():
            raise ValueError("Model not fitted.")
        if rb.num_rows < self._order:
            raise ValueError(f"Not enough information. There are less rows in test DataFrame ({rb.num_rows}) than the markovian "
                             f"order of the DynamicBayesianNetwork ({self._order})")

    def logl(self, df):
        """DynamicBayesianNetwork::logl (DynamicBayesianNetwork.cpp:71-113): the first `order` rows from the static
        network (row i scored by the factors of slice order - i), the rest from the transition network."""
        rb = as_record_batch(df)
        self._check(rb)
        ll = np.zeros(rb.num_rows)
        dstatic = static_table(rb.slice(0, self._order), self._order)
        for i in range(self._order):
            for v in self._variables:
                ll[i] += self._static.cpd(temporal_name(v, self._order - i)).slogl(dstatic)
        if rb.num_rows > self._order:
            dtrans = transition_table(rb, self._order)
            whole = self._transition_in_one_pass(dtrans, "logl")
            if whole is not None:   # the same adds: 0 + (ll_0 + ll_1 + ...) carries the bits of ((0 + ll_0) + ll_1) + ...
                ll[self._order:] += whole
            else:
                for v in self._variables:
                    ll[self._order:] += self._transition.cpd(temporal_name(v, 0)).logl(dtrans)
        return ll

    def _transition_in_one_pass(self, dtrans, what):
        """The transition network's "logl" (per row) or "slogl" (per node) over `dtrans` in one pass, or None: gaussian_model.py when all
        its factors are exactly LinearGaussianCPD, clg_model.py when they are DiscreteFactors and (C)LinearGaussianCPDs of both kinds -
        and its node order is the order this class adds the variables' values in.  Known gap: the discrete pass is not asked, so an
        all-DiscreteFactor transition network stays on the per-factor loop."""
        t = self._transition
        if list(t._nodes) != [temporal_name(v, 0) for v in self._variables]:
            return None
        served = one_pass(t, dtrans, what, only=(GAUSSIAN, CLG))
        return None if served is None else served.value

    def slogl(self, df):
        rb = as_record_batch(df)
        self._check(rb)
        total = 0.0
        dstatic = static_table(rb.slice(0, self._order), self._order)
        for i in range(self._order):
            for v in self._variables:
                total += self._static.cpd(temporal_name(v, self._order - i)).slogl(dstatic)
        if rb.num_rows > self._order:
            dtrans = transition_table(rb, self._order)
            per_node = self._transition_in_one_pass(dtrans, "slogl")
            if per_node is not None:
                for s in per_node:
                    total += float(s)
            else:
                for v in self._variables:
                    total += self._transition.cpd(temporal_name(v, 0)).slogl(dtrans)
        return total

    def sample(self, n, seed=None):
        """DynamicBayesianNetwork::sample (DynamicBayesianNetwork.cpp:153-466): the first `markovian_order` rows are ONE
        sample of the static network (row i is slice order - i), every later row i is drawn variable by variable in the
        transition network's topological order, each factor sampling one value given the window of rows i-order .. i
        with seed + i.  Returns a pyarrow.RecordBatch over variables()."""
        import pyarrow as pa

        from .factors import _random_seed

        if not self.fitted():
            raise ValueError("DynamicBayesianNetwork currently not fitted. Call fit() method, or add_cpds() for static_bn() and transition_bn()")
        if n < 0:
            raise ValueError("n should be a non-negative number")
        seed = _random_seed() if seed is None else int(seed)
        order = self._order
        types, cats, cols = {}, {}, {}
        for v in self._variables:   # check_same_datatypes + generate_empty_dataframe
            cpd0 = self._transition.cpd(temporal_name(v, 0))
            dt = cpd0.data_type()
            for i in range(1, order + 1):
                other = self._static.cpd(temporal_name(v, i)).data_type()
                if pa.types.is_dictionary(dt) != pa.types.is_dictionary(other) or (not pa.types.is_dictionary(dt) and dt != other):
                    raise ValueError(f"Data type for transition Bayesian network node {temporal_name(v, 0)} [{dt}] is different from data "
                                     f"type of static Bayesian network node {temporal_name(v, i)}[{other}]")
            types[v] = dt
            if pa.types.is_dictionary(dt):
                cats[v] = list(cpd0._categories[0])
                for i in range(1, order):
                    if list(self._static.cpd(temporal_name(v, i))._categories[0]) != cats[v]:
                        raise ValueError(f"CPD of transition Bayesian network node {temporal_name(v, 0)} have different categories than "
                                         f"static Bayesian network node {temporal_name(v, i)}.")
                cols[v] = np.zeros(n, dtype=np.int64)
            elif dt == pa.float64() or dt == pa.float32():
                cols[v] = np.zeros(n, dtype=np.float64 if dt == pa.float64() else np.float32)
            else:
                raise ValueError("Data type not supported for sampling.")

        def scalar(arr):
            if isinstance(arr, pa.ChunkedArray):
                arr = arr.combine_chunks()
            if pa.types.is_dictionary(arr.type):
                return int(arr.indices[0].as_py())
            return arr[0].as_py()

        static_sample = self._static.sample(1, seed & 0xFFFFFFFF)
        for v in self._variables:
            for i in range(min(order, n)):
                cols[v][i] = scalar(static_sample.column(static_sample.schema.get_field_index(temporal_name(v, order - i))))

        def window_value(name, i):   # column `name` = v_t_k of the one-row transition table of rows i-order .. i
            v, k = name.rsplit("_t_", 1)
            val = cols[v][i - int(k)]
            if v in cats:
                return pa.DictionaryArray.from_arrays(pa.array([int(val)], type=pa.int32()), pa.array(cats[v]))
            return pa.array(np.asarray([val], dtype=cols[v].dtype))

        top_sort = self._transition.topological_sort()
        for i in range(order, n):
            for full in top_sort:
                cpd = self._transition.cpd(full)
                ev = cpd.evidence()
                evidence = pa.RecordBatch.from_arrays([window_value(e, i) for e in ev], names=list(ev)) if ev else None
                cols[full[:-4]][i] = scalar(cpd.sample(1, evidence, (seed + i) & 0xFFFFFFFF))
        arrays = []
        for v in self._variables:
            if v in cats:
                arrays.append(pa.DictionaryArray.from_arrays(pa.array(cols[v], type=pa.int64()).cast(types[v].index_type), pa.array(cats[v])))
            else:
                arrays.append(pa.array(cols[v]))
        return pa.RecordBatch.from_arrays(arrays, names=list(self._variables))

    @property
    def include_cpd(self):
        return bool(self._static.include_cpd and self._transition.include_cpd)

    @include_cpd.setter
    def include_cpd(self, value):
        self._static.include_cpd = self._transition.include_cpd = bool(value)

    def save(self, name, include_cpd=False):
        import pickle

        self.include_cpd = include_cpd
        with open(name if name.endswith(".pickle") else name + ".pickle", "wb") as f:
            pickle.dump(self, f, protocol=2)

    def __getstate__(self):
        """DynamicBayesianNetwork::__getstate__ (DynamicBayesianNetwork.hpp:160-190): variables, order and the two
        networks (which carry their factors when include_cpd is set); a Python-derived class adds __getstate_extra__()."""
        state = {"variables": self._variables, "order": self._order, "static": self._static, "transition": self._transition}
        extra = getattr(self, "__getstate_extra__", None)
        if extra is not None:
            state["extra"] = extra()
        return state

    def __setstate__(self, state):
        self._variables, self._order = list(state["variables"]), state["order"]
        self._static, self._transition = state["static"], state["transition"]
        if "extra" in state:
            self.__setstate_extra__(state["extra"])

    def __str__(self):
        return f"Dynamic{self.type()} of order {self._order} over {len(self._variables)} variables"

    __repr__ = __str__


def _typed_dbn(name, type_name, message, doc):
    def __init__(self, variables, markovian_order, static_bn=None, transition_bn=None):
        from . import models

        bn_type = getattr(models, type_name)()
        if static_bn is not None and transition_bn is not None and static_bn.type() != transition_bn.type():
            raise ValueError("Static and transition Bayesian networks do not have the same type.")
        for bn in (static_bn, transition_bn):
            if bn is not None and bn.type() != bn_type:
                raise ValueError(message)
        DynamicBayesianNetwork.__init__(self, variables, markovian_order, static_bn, transition_bn, bn_type=bn_type)

    return type(name, (DynamicBayesianNetwork,), {"__init__": __init__, "__doc__": doc, "__module__": __name__})


DynamicGaussianNetwork = _typed_dbn("DynamicGaussianNetwork", "GaussianNetworkType", "Bayesian networks are not Gaussian.",
                                    "models/DynamicBayesianNetwork.hpp: dynamic GaussianNetwork.")
DynamicSemiparametricBN = _typed_dbn("DynamicSemiparametricBN", "SemiparametricBNType", "Bayesian networks are not semiparametric.",
                                     "Dynamic SemiparametricBN.")
DynamicKDENetwork = _typed_dbn("DynamicKDENetwork", "KDENetworkType", "Bayesian networks are not KDE networks.", "Dynamic KDENetwork.")
DynamicDiscreteBN = _typed_dbn("DynamicDiscreteBN", "DiscreteBNType", "Bayesian networks are not discrete.", "Dynamic DiscreteBN.")
DynamicCLGNetwork = _typed_dbn("DynamicCLGNetwork", "CLGNetworkType", "Bayesian networks are not CLG networks.", "Dynamic CLGNetwork.")


class DynamicHomogeneousBN(DynamicBayesianNetwork):
    def __init__(self, factor_type, variables, markovian_order):
        from .models import HomogeneousBNType

        DynamicBayesianNetwork.__init__(self, HomogeneousBNType(factor_type), variables, markovian_order)


class DynamicHeterogeneousBN(DynamicBayesianNetwork):
    def __init__(self, factor_types, variables, markovian_order):
        from .models import HeterogeneousBNType

        DynamicBayesianNetwork.__init__(self, HeterogeneousBNType(factor_types), variables, markovian_order)


def static_blacklist(variables, markovian_order):
    """dmmhc.cpp:12-32: in the static network no arc may run from a more recent slice to an older one."""
    if markovian_order == 1:
        return []
    slices = [[temporal_name(v, i) for v in variables] for i in range(1, markovian_order + 1)]
    out = []
    for i in range(markovian_order - 1):
        for source in slices[i]:
            for j in range(i + 1, markovian_order):
                out += [(source, dest) for dest in slices[j]]
    return out


class DMMHC:
    """learning/algorithms/dmmhc.cpp:34-118: MMHC on the static table, conditional MMHC on the transition table."""

    def estimate(self, hypot_test, operators, score, variables=(), bn_type=None, markovian_order=1, static_callback=None,
                 transition_callback=None, max_indegree=0, max_iters=2 ** 31 - 1, epsilon=0.0, patience=0, alpha=0.05, verbose=0):
        from .learning import MMHC

        bn_type = bn_type if bn_type is not None else GaussianNetworkType()
        variables = list(variables) if variables else list(hypot_test.variable_names())
        if not hypot_test.has_variables(variables):
            raise ValueError("DynamicIndependenceTest do not contain all the variables in nodes lists.")
        if not score.has_variables(variables):
            raise ValueError("Score do not contain all the variables in nodes list.")
        mmhc = MMHC()
        static_nodes = temporal_names(variables, 1, markovian_order)
        g0 = mmhc.estimate(hypot_test.static_tests(), operators, score.static_score(), static_nodes, bn_type,
                           arc_blacklist=static_blacklist(variables, markovian_order), callback=static_callback,
                           max_indegree=max_indegree, max_iters=max_iters, epsilon=epsilon, patience=patience, alpha=alpha)
        self.static_tests, self.static_cpcs, self.static_search = mmhc.last_tests, mmhc.last_cpcs, mmhc.hc.last
        transition_nodes = temporal_names(variables, 0, 0)
        gt = mmhc.estimate_conditional(hypot_test.transition_tests(), operators, score.transition_score(), transition_nodes,
                                       static_nodes, bn_type, callback=transition_callback, max_indegree=max_indegree,
                                       max_iters=max_iters, epsilon=epsilon, patience=patience, alpha=alpha)
        self.transition_tests, self.transition_cpcs, self.transition_search = mmhc.last_tests, mmhc.last_cpcs, mmhc.hc.last
        return DynamicBayesianNetwork(variables, markovian_order, g0, gt)
